"""Independent numpy (float64) restatement of the splat pipeline in conventional math form.

Purpose: catch transcription errors in oracle/gs_oracle.c (a transposed matrix, a wrong SH sign, a
swapped conic entry).  It is written from the GLSL shaders via the "conventional math" reading in
SURVEY.md Appendix A -- standard rotation matrix, Sigma = R S^2 R^T, cov2d = (J V) Sigma (J V)^T --
NOT by following the oracle's column-major emulation, and it evaluates in float64 with numpy's own
exp.  So it agrees with the oracle to ~1e-6 relative, not bit for bit; discrete decisions may flip for
the rare value sitting on a threshold, which the tests allow for explicitly.
"""
import numpy as np

# Every constant of the shaders' decisions, named.  preprocess()/render() and what follows take `rules=` overrides of these
# (tests/test_float64_edges.py perturbs each one and demands that the float64 check notices); the defaults are the shaders'.
RULES = dict(
    near=0.2,              # preprocess.comp:135  cull p_view.z <= near
    frustum=1.3,           # preprocess.comp:40-41 Jacobian clamp of tx/tz, ty/tz at frustum * tan(fov/2)
    dilation=0.3,          # preprocess.comp:63-64 added to the 2D covariance's diagonal
    floor=0.1,             # preprocess.comp:149  max(floor, mid^2 - det)
    radius=3.0,            # preprocess.comp:152  ceil(radius * sqrt(lambda))
    tile_round=15,         # preprocess.comp:163  (uv + r + tile_round) / 16
    uv_offset=1.0,         # preprocess.comp:112  ((v + 1) S - uv_offset) / 2
    clamp_channels=(0,),   # preprocess.comp:102  only red is clamped at 0
    alpha_max=0.99,        # render.comp:77
    alpha_min=1.0 / 255.0,  # render.comp:78
    T_cut=1e-4,            # render.comp:83
    tie=1,                 # equal depth bits: +1 ids ascending (a stable sort of the 64-bit keys), -1 descending
    f2i="saturate",        # preprocess.comp:161-164 int() of a box coordinate beyond int32 (GLSL leaves it undefined; the
                           # pipeline saturates): "saturate", or "wrap" (modulo 2^32, what a bare conversion may give)
)


def rules_with(rules=None):
    r = dict(RULES)
    if rules:
        unknown = set(rules) - set(RULES)
        assert not unknown, unknown
        r.update(rules)
    return r

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
         -0.4570457994644658, 1.445305721320277, -0.5900435899266435]


def activate(records, sh16=False):
    """GSScene.cpp:36-59 -> dict of float64 arrays.  sh16: the coefficients as the opt-in binary16 SH storage holds them
    (each rounded to the nearest binary16, ties to even, as Scene.quantize_sh stores them)."""
    r = records.astype(np.float64)
    sh_planar = r[:, 6:54]
    if sh16:
        sh_planar = sh_planar.astype(np.float16).astype(np.float64)
    sh = np.zeros((len(r), 16, 3))
    sh[:, 0, :] = sh_planar[:, 0:3]
    for c in range(3):
        sh[:, 1:, c] = sh_planar[:, 3 + 15 * c: 3 + 15 * (c + 1)]
    rot = r[:, 58:62]
    return dict(pos=r[:, 0:3], scale=np.exp(r[:, 55:58]), opacity=1.0 / (1.0 + np.exp(-r[:, 54])),
                rot=rot / np.linalg.norm(rot, axis=1, keepdims=True), sh=sh)


def rotation_std(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - z * w)
    R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w)
    R[:, 2, 1] = 2 * (y * z + x * w)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def cov3d(scene):
    R = rotation_std(scene["rot"])
    S2 = scene["scale"] ** 2
    Sigma = np.einsum("nij,nj,nkj->nik", R, S2, R)  # R S^2 R^T
    return Sigma


def camera(position, quat, fov_deg, near, far, width, height):
    """Renderer.cpp:719-754 in conventional form: world->camera, then the row flips."""
    w, x, y, z = quat
    Rc = rotation_std(np.array([[w, x, y, z]], dtype=np.float64))[0]
    M = np.eye(4)
    M[:3, :3] = Rc
    M[:3, 3] = position
    V0 = np.linalg.inv(M)
    tan_fovx = np.tan(np.radians(fov_deg) / 2.0)
    tan_fovy = tan_fovx * height / width
    P = np.zeros((4, 4))
    P[0, 0] = 1.0 / ((width / height) * tan_fovy)
    P[1, 1] = 1.0 / tan_fovy
    P[2, 2] = -(far + near) / (far - near)
    P[2, 3] = -(2.0 * far * near) / (far - near)
    P[3, 2] = -1.0
    proj = np.diag([1.0, -1.0, 1.0, 1.0]) @ P @ V0
    view = np.diag([1.0, -1.0, -1.0, 1.0]) @ V0
    return dict(proj=proj, view=view, tan_fovx=tan_fovx, tan_fovy=tan_fovy, cam=np.asarray(position, float),
                width=width, height=height)


def preprocess(scene, cam, rules=None):
    R = rules_with(rules)
    W, H = cam["width"], cam["height"]
    n = len(scene["pos"])
    ph = np.concatenate([scene["pos"], np.ones((n, 1))], axis=1)
    p_hom = ph @ cam["proj"].T
    p_view = ph @ cam["view"].T
    ndc = p_hom[:, :2] / p_hom[:, 3:4]
    tz = p_view[:, 2]
    vis = tz > R["near"]
    tzs = np.where(vis, tz, 1.0)
    limx, limy = R["frustum"] * cam["tan_fovx"], R["frustum"] * cam["tan_fovy"]
    tx = np.clip(p_view[:, 0] / tzs, -limx, limx) * tzs
    ty = np.clip(p_view[:, 1] / tzs, -limy, limy) * tzs
    fx, fy = W / (2 * cam["tan_fovx"]), H / (2 * cam["tan_fovy"])
    Jac = np.zeros((n, 2, 3))
    Jac[:, 0, 0] = fx / tzs
    Jac[:, 0, 2] = -fx * tx / tzs ** 2
    Jac[:, 1, 1] = fy / tzs
    Jac[:, 1, 2] = -fy * ty / tzs ** 2
    A = Jac @ cam["view"][:3, :3]
    cov2 = A @ cov3d(scene) @ np.transpose(A, (0, 2, 1))
    a, b, c = cov2[:, 0, 0] + R["dilation"], cov2[:, 0, 1], cov2[:, 1, 1] + R["dilation"]
    det = a * c - b * b
    vis &= det > 0
    dets = np.where(vis, det, 1.0)
    conic = np.stack([c / dets, -b / dets, a / dets], axis=1)
    mid = 0.5 * (a + c)
    lam = mid + np.sqrt(np.maximum(R["floor"], mid * mid - det))
    radius = np.ceil(R["radius"] * np.sqrt(np.maximum(lam, 0)))
    uv = ((ndc + 1.0) * np.array([W, H]) - R["uv_offset"]) * 0.5
    box = box_coords(box_args(uv, radius, R), W, H, R)
    tiles = np.where(vis, box_tiles(box, R), 0)
    # SH
    d = scene["pos"] - cam["cam"]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    sh = scene["sh"]
    rgb = SH_C0 * sh[:, 0] - SH_C1 * y * sh[:, 1] + SH_C1 * z * sh[:, 2] - SH_C1 * x * sh[:, 3]
    rgb += SH_C2[0] * x * y * sh[:, 4] + SH_C2[1] * y * z * sh[:, 5] + SH_C2[2] * (2 * z * z - x * x - y * y) * sh[:, 6]
    rgb += SH_C2[3] * z * x * sh[:, 7] + SH_C2[4] * (x * x - y * y) * sh[:, 8]
    rgb += SH_C3[0] * (3 * x * x - y * y) * y * sh[:, 9] + SH_C3[1] * x * y * z * sh[:, 10]
    rgb += SH_C3[2] * (4 * z * z - x * x - y * y) * y * sh[:, 11]
    rgb += SH_C3[3] * z * (2 * z * z - 3 * x * x - 3 * y * y) * sh[:, 12]
    rgb += SH_C3[4] * x * (4 * z * z - x * x - y * y) * sh[:, 13]
    rgb += SH_C3[5] * (x * x - y * y) * z * sh[:, 14] + SH_C3[6] * x * (x * x - 3 * y * y) * sh[:, 15]
    rgb += 0.5
    for k in R["clamp_channels"]:
        rgb[:, k] = np.maximum(rgb[:, k], 0.0)
    return dict(tiles=tiles, box=box, conic=conic, radius=radius, uv=uv, depth=tz, rgb=rgb, opacity=scene["opacity"],
                cov2d=np.stack([a, b, c], axis=1), mid=mid, det=det, lam=lam,
                cov_scale=(A ** 2).sum(axis=(1, 2)) * scene["scale"].max(axis=1) ** 2)  # |J W|_F^2 |Sigma|: of the 2D covariance's terms


def render(pre, width, height, rules=None):
    """Straight per-pixel blend over depth-sorted Gaussians (tile membership through the boxes)."""
    R = rules_with(rules)
    vis = np.nonzero(pre["tiles"])[0]
    order = vis[np.lexsort((R["tie"] * vis, pre["depth"][vis].astype(np.float32).view(np.uint32)))]
    img = np.zeros((height, width, 4))
    img[..., 3] = 1.0
    T = np.ones((height, width))
    alive = np.ones((height, width), bool)
    ys, xs = np.mgrid[0:height, 0:width]
    for g in order:
        x0, y0, x1, y1 = pre["box"][g]
        sl = (slice(y0 * 16, min(y1 * 16, height)), slice(x0 * 16, min(x1 * 16, width)))
        dx = pre["uv"][g, 0] - xs[sl]
        dy = pre["uv"][g, 1] - ys[sl]
        c00, c01, c11 = pre["conic"][g]
        power = -0.5 * (c00 * dx * dx + c11 * dy * dy) - c01 * dx * dy
        alpha = np.minimum(R["alpha_max"], pre["opacity"][g] * np.exp(np.minimum(power, 0)))
        ok = alive[sl] & (power <= 0) & (alpha >= R["alpha_min"])
        test_T = T[sl] * (1 - alpha)
        kill = ok & (test_T < R["T_cut"])
        upd = ok & ~kill
        for k in range(3):
            img[sl + (k,)] += np.where(upd, pre["rgb"][g, k] * alpha * T[sl], 0.0)
        T[sl] = np.where(upd, test_T, T[sl])
        alive[sl] &= ~kill
    return img


def box_args(uv, radius, rules=None):
    """preprocess.comp:161-164: the four values the tile box converts to int, (n, 4): x0, y0, x1, y1."""
    R = rules_with(rules)
    return np.stack([(uv[:, 0] - radius) / 16, (uv[:, 1] - radius) / 16, (uv[:, 0] + radius + R["tile_round"]) / 16,
                     (uv[:, 1] + radius + R["tile_round"]) / 16], axis=1)


def box_coords(args, width, height, rules=None):
    """int() of box_args (truncation; beyond int32 by the f2i rule), clamped to the tile grid."""
    R = rules_with(rules)
    tw, th = (width + 15) // 16, (height + 15) // 16
    with np.errstate(invalid="ignore"):
        t = np.trunc(args)
        if R["f2i"] == "wrap":
            t = np.mod(t + 2.0 ** 31, 2.0 ** 32) - 2.0 ** 31
        else:
            assert R["f2i"] == "saturate", R["f2i"]  # (the clamp below does what saturation would)
        return np.nan_to_num(np.clip(t, 0, np.array([tw, th, tw, th]))).astype(np.int64)


def box_tiles(box, rules=None):
    """preprocess.comp:169: the number of tiles of a box, in uint32 arithmetic (a box with x1 < x0 is NOT empty there)."""
    R = rules_with(rules)
    if R["f2i"] == "saturate":  # x1 >= x0 and y1 >= y0 always: no wrap-around to model
        return (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    m = np.uint64(0xFFFFFFFF)
    wx = (box[:, 2] - box[:, 0]).astype(np.uint64) & m
    wy = (box[:, 3] - box[:, 1]).astype(np.uint64) & m
    return ((wx * wy) & m).astype(np.int64)


def tile_lists(pre, width, height, rules=None):
    """Binning and depth order restated without the radix sort or the LDS sort: every visible Gaussian is listed in each tile of
    its box; the lists are tile-major, then ascending by the binary32 bit pattern of the depth (what the 64-bit keys
    preprocess_sort.comp builds compare), then by id (a stable sort).  Returns (tile of each entry, id of each entry, ranges)
    with ranges[2 t], ranges[2 t + 1] = [start, end) of tile t (tile_boundary.comp), as the stage taps hold them."""
    R = rules_with(rules)
    tw, th = (width + 15) // 16, (height + 15) // 16
    vis = np.nonzero(np.asarray(pre["tiles"]) > 0)[0]
    box = np.asarray(pre["box"], np.int64)[vis]
    counts = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    gid = np.repeat(vis, counts)
    start = np.repeat(np.cumsum(counts) - counts, counts)
    k = np.arange(len(gid)) - start                       # the entry's index inside its own box, row-major
    bw = np.repeat(box[:, 2] - box[:, 0], counts)
    tile = (np.repeat(box[:, 1], counts) + k // np.maximum(bw, 1)) * tw + np.repeat(box[:, 0], counts) + k % np.maximum(bw, 1)
    bits = np.asarray(pre["depth"], np.float32)[gid].view(np.uint32).astype(np.int64)
    order = np.lexsort((R["tie"] * gid, bits, tile))
    tile, gid = tile[order], gid[order]
    ranges = np.zeros(2 * tw * th, np.int64)
    first = np.searchsorted(tile, np.arange(tw * th), side="left")
    last = np.searchsorted(tile, np.arange(tw * th), side="right")
    ranges[0::2] = np.where(last > first, first, 0)
    ranges[1::2] = np.where(last > first, last, 0)
    return tile, gid, ranges


def blend(att, gid, ranges, width, height, rules=None, err=None):
    """render.comp over given lists, in float64, vectorised per tile (the decisions of render(), entry by entry).
    att: uv (N, 2), conic (N, 3), opacity (N), rgb (N, 3).  gid, ranges: the lists (tile_lists()).
    Also returns, per pixel, how close the pixel's list comes to each of the blend's decisions ("distance to a decision", as
    helpers.classify_pixel measures it for binary32 lists) once the uncertainty of the binary32 inputs being compared is
    taken off.  err: per-Gaussian uncertainties (all optional, default 0): "conic" absolute per conic entry, "uv" absolute per
    coordinate, "rel" of `power` relative to its terms (rounding), "alpha" relative (exp(), opacity), "rgb" absolute.
    dec["power"]: min over the reached entries of |power| - d_power (0: the `power > 0` skip may flip);
    dec["alpha"]: min of |alpha / alpha_min - 1| - d_alpha (0: the alpha cut may flip);
    dec["T"]: min of |test_T / T_cut - 1| - the relative uncertainty of T accumulated so far (0: the T cut may flip);
    dec["cancel"]: first-order bound of how far the pixel moves when no decision flips."""
    R = rules_with(rules)
    n = len(att["opacity"])
    E = {k: np.zeros(n) for k in ("conic", "uv", "rel", "alpha", "rgb")}
    E.update({k: np.asarray(v, np.float64) for k, v in (err or {}).items()})
    tw = (width + 15) // 16
    img = np.zeros((height, width, 4))
    img[..., 3] = 1.0
    dec = {k: np.full((height, width), np.inf) for k in ("alpha", "T", "power")}
    dec["cancel"] = np.zeros((height, width))
    uv, co, op, rgb = att["uv"], att["conic"], att["opacity"], att["rgb"]
    for t in range(len(ranges) // 2):
        s, e = int(ranges[2 * t]), int(ranges[2 * t + 1])
        if e <= s:
            continue
        ty, tx = divmod(t, tw)
        ys, xs = np.mgrid[ty * 16:min(ty * 16 + 16, height), tx * 16:min(tx * 16 + 16, width)]
        py, px = ys.ravel().astype(np.float64), xs.ravel().astype(np.float64)
        ids = gid[s:e]
        dx = uv[ids, 0:1] - px[None, :]
        dy = uv[ids, 1:2] - py[None, :]
        c00, c01, c11 = co[ids, 0:1], co[ids, 1:2], co[ids, 2:3]
        t1, t2, t3 = c00 * dx * dx, c11 * dy * dy, c01 * dx * dy
        power = -0.5 * (t1 + t2) - t3
        alpha = np.minimum(R["alpha_max"], op[ids, None] * np.exp(np.minimum(power, 0.0)))
        ok = (power <= 0) & (alpha >= R["alpha_min"])
        f = np.where(ok, 1.0 - alpha, 1.0)
        T_ex = np.ones_like(f)
        if len(ids) > 1:
            T_ex[1:] = np.cumprod(f, axis=0)[:-1]
        test_T = T_ex * (1.0 - alpha)
        kill = ok & (test_T < R["T_cut"])
        m = len(ids)
        stop = np.where(kill.any(axis=0), kill.argmax(axis=0), m)      # the entry at which the pixel breaks (m: none)
        k = np.arange(m)[:, None]
        used = ok & (k < stop[None, :])
        reached = k <= stop[None, :]
        w = np.where(used, alpha * T_ex, 0.0)
        c = w.T @ rgb[ids]                                               # (P, 3)
        # what the binary32 inputs' uncertainty can move `power` by, absolutely, and alpha, relatively
        mag = 0.5 * (np.abs(t1) + np.abs(t2)) + np.abs(t3)
        dp = (E["rel"][ids, None] * mag + E["conic"][ids, None] * (0.5 * (dx * dx + dy * dy) + np.abs(dx * dy))
              + E["uv"][ids, None] * (np.abs(c00 * dx + c01 * dy) + np.abs(c01 * dx + c11 * dy)))
        da = np.where(alpha < R["alpha_max"], dp, 0.0) + E["alpha"][ids, None]
        pw = np.where(reached, np.maximum(0.0, np.abs(power) - dp), np.inf)
        al = np.where(reached & (power <= 0), np.maximum(0.0, np.abs(alpha / R["alpha_min"] - 1.0) - da), np.inf)
        t_err = np.cumsum(np.where(ok & reached, da * alpha / np.maximum(1.0 - alpha, 1e-2), 0.0), axis=0) + 4.0 * 2.0 ** -24 * (k + 1)
        Td = np.where(ok & reached, np.maximum(0.0, np.abs(test_T / R["T_cut"] - 1.0) - t_err), np.inf)
        rmax = np.abs(rgb[ids]).max(axis=1)
        cancel = (w * (da * (rmax[:, None] + rmax.max()) + E["rgb"][ids, None])).sum(axis=0)
        sl = (ys, xs)
        img[sl + (slice(0, 3),)] = c.reshape(ys.shape + (3,))
        dec["power"][sl] = pw.min(axis=0).reshape(ys.shape)
        dec["alpha"][sl] = al.min(axis=0).reshape(ys.shape)
        dec["T"][sl] = Td.min(axis=0).reshape(ys.shape)
        dec["cancel"][sl] = cancel.reshape(ys.shape)
    return img, dec


def bgra8(rgba):
    """The BGRA8 frame of an RGBA image, as the oracle restates the reference's UNORM conversion (gso_pack_bgra8): each channel
    clamped to [0, 1] (NaN -> 0), times 255, rounded to nearest with ties to even; channels stored B, G, R, A.  In float64:
    the product x * 255 is exact here, where the binary32 product rounds -- the two can differ only where x * 255 lies within
    one binary32 rounding of a half-integer (what bgra8_tie() marks)."""
    x = np.nan_to_num(np.asarray(rgba, np.float64), nan=0.0)
    q = np.rint(np.clip(x, 0.0, 1.0) * 255.0).astype(np.uint8)
    return q[..., [2, 1, 0, 3]]


def bgra8_tie(rgba, slack):
    """Per BGRA channel: True where x * 255 (x clamped) lies within `slack` (absolute, in units of x) of a rounding boundary."""
    x = np.clip(np.nan_to_num(np.asarray(rgba, np.float64), nan=0.0), 0.0, 1.0) * 255.0
    near = np.abs(x - np.floor(x) - 0.5) <= np.asarray(slack, np.float64) * 255.0
    return near[..., [2, 1, 0, 3]]
