"""The yardstick of gs_project_backward (include/gs3d_hip.h): the definition restated in numpy binary64.

THE FUNCTION.  For a visible Gaussian with stored binary32 position p, activated scale s, stored quaternion q (w x y z), activated
opacity o and the 16 x 3 SH coefficients as stored, and the frame's uniforms, the screen-space record is the exact real function F
the header writes down (h, t, u v, the clamped tx ty, J, A = J V, Sigma = R(q^) diag(s^2) R(q^)^T, cov = A Sigma A^T, the 0.3
dilation, det, the conic, comp in antialiased frames, the view direction d and the sixteen basis polynomials).  Every constant is
the frame's binary32 constant converted exactly: 1.3f * tan_fov (the binary32 product), 0.3f, 0.5f, the SH constants of sh_to_rgb.
This module computes, per parameter theta, sum_x g_x dx/dtheta over the nine record values x by the chain rule, node by node:
    conic -> (m00, m01, m11, det) -> cov (+ comp's det_raw and det in antialiased frames) -> M = A R -> s^2, R, A -> J -> t;
    t -> p through the view matrix;  uv -> p through h;  rgb -> sh directly and -> d -> p;  R -> q^ -> q;  s -> log s;  o -> logit.
Three things are NOT computed here but taken from the frame, as constants: which Gaussians are visible (oracle.stages(...)["tiles"]
!= 0), whether channel 0 flows (the oracle's colour r > 0), and the branch of each clamp -- a numpy-binary32 restatement of the
p_view rows and the one division of k_preprocess (clamp_branches below; its p_view[2] is the oracle's depth bit for bit:
tests/test_project_backward_api.py).

THE BOUND.  The definition leaves the association open, so the contract is a bound.  Every quantity here is carried as a triple
(value, magnitude, count) -- class V -- with the rules
    exact input x:   (x, |x|, 0)
    a + b, a - b:    (.., mag a + mag b,              max(k_a, k_b) + 1)
    a * b:           (.., mag a * mag b,              k_a + k_b + 1)
    a / b:           (.., mag a * mag b / b^2,        k_a + k_b + 1)       mag b / |b| is b's condition factor: it rides along
    sqrt(a):         (.., mag a / sqrt(a),            k_a + 1)
    2 a, a / 2, -a, a select:  exact, nothing changes
so mag >= |value| always, every input gradient, partial and product enters by its absolute value, and the condition factor of each
cancelling intermediate that is divided by (h3, t2, det, det_raw, comp, |p - c|) or multiplied with (the cov2D entries, the basis
polynomials) is carried into everything downstream.  By induction over the rules, with u = 2^-53 and to first order: a quantity
computed in binary64 from exact inputs, by these operations in ANY association of its sums and products, differs from its exact
value by at most  k u mag  -- a sum of n terms costs at most n - 1 more roundings than its worst term whatever the order, which is
what the sequential sums here count; a product of n factors costs the factors' counts plus n - 1 in every order.  k is counted by
the arithmetic itself on the longest path to each output -- 657 for a quaternion's gradient in an antialiased frame, 650 and 637 for
a mean's and a log-scale's, 320 for an opacity logit's, 31 for an SH coefficient's: relative errors add through products, and the
chain from a conic to a quaternion is some forty factors deep -- and K_PATH = 660 bounds them all (asserted on every call).
Both sides of a comparison lie within that of the exact value, so for every element
    |got - want| <= 2 K_PATH 2^-53 A            A = the element's magnitude
and after `times` calls into an array preloaded with x:  2 times ((K_PATH + times) A + |x|) 2^-53  (each add is one more rounding
of a content of at most |x| + times A).  A statement about arithmetic, not a fitted tolerance.  Where A is 0 -- every gradient
that reaches the element is an exact zero -- the element keeps its bits.

`mutate` names single-term mutations of the chain; the tests show that each moves some element by more than 1000 bounds.
A plain module: numpy only (the oracle's outputs come in as arrays)."""
import numpy as np

U53 = 2.0 ** -53
K_PATH = 660
OUTPUTS = {"means": (3,), "log_scales": (3,), "quats": (4,), "opacity_logits": (), "sh_dc": (3,), "sh_rest": None}   # sh_rest: (K, 3)
INPUTS = {"colour": (3,), "opacity": (), "conic": (3,), "uv": (2,)}
MUTATIONS = ("no_direction", "clamp_is_constant", "no_tangent_projection", "no_comp_cov", "red_always_flows", "s_not_squared",
             "view_transposed", "view_transposed_in_a", "view_transposed_in_g_j", "camera_at_origin")
# the last four are invisible under a camera at the origin with a symmetric view rotation (the default one): each of the first three
# reads the view matrix's 3 x 3 block transposed in ONE of its uses (g_p <- g_t; A = J V; g_Jaa, g_Ja2 <- g_A), the fourth takes the
# view direction from p instead of p - camera_position.  tests/test_backward_cameras_api.py asserts both halves of that.
RECORD = {"uv": 2, "conic": 3, "opacity": 1, "rgb_raw": 3, "rgb": 3}

_F = np.float32
SH_C0, SH_C1 = float(_F(0.28209479177387814)), float(_F(0.4886025119029199))
SH_C2 = [float(_F(c)) for c in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)]
SH_C3 = [float(_F(c)) for c in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                                -0.4570457994644658, 1.445305721320277, -0.5900435899266435)]
DILATION = float(_F(0.3))


class V:
    """(value, magnitude, rounding count) under the rules of the module's docstring; vectorised over the Gaussians."""
    __slots__ = ("v", "m", "k")

    def __init__(self, v, m=None, k=0):
        self.v = np.asarray(v, np.float64)
        self.m = np.abs(self.v) if m is None else np.asarray(m, np.float64)
        self.k = k

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(a, b):
        b = V.of(b)
        return V(a.v + b.v, a.m + b.m, max(a.k, b.k) + 1)

    __radd__ = __add__

    def __sub__(a, b):
        b = V.of(b)
        return V(a.v - b.v, a.m + b.m, max(a.k, b.k) + 1)

    def __rsub__(a, b):
        return V.of(b) - a

    def __neg__(a):
        return V(-a.v, a.m, a.k)

    def __mul__(a, b):
        b = V.of(b)
        return V(a.v * b.v, a.m * b.m, a.k + b.k + 1)

    __rmul__ = __mul__

    def __truediv__(a, b):
        b = V.of(b)
        return V(a.v / b.v, a.m * b.m / (b.v * b.v), a.k + b.k + 1)

    def __rtruediv__(a, b):
        return V.of(b) / a

    def sqrt(a):
        r = np.sqrt(a.v)
        return V(r, a.m / r, a.k + 1)

    def pow2(a, e):
        """a * 2^e: exact."""
        return V(a.v * 2.0 ** e, a.m * 2.0 ** e, a.k)

    def where(a, cond, b):
        """a where cond, else b: a selection, never a product with zero."""
        b = V.of(b)
        return V(np.where(cond, a.v, b.v), np.where(cond, a.m, b.m), max(a.k, b.k))


def _sum(terms):
    out = terms[0]
    for t in terms[1:]:
        out = out + t
    return out


def unpack_vertices(verts, sh16=False):
    """(pos, scale, quat, opacity, sh [n][16][3]) float32 from the oracle's activated vertices (or Scene.download_vertices viewed so);
    sh16: the coefficients as Scene.quantize_sh stores them."""
    if verts.dtype.names is None:
        flat = np.ascontiguousarray(verts, np.float32).reshape(-1, 60)
        pos, so, rot, sh = flat[:, 0:3], flat[:, 4:8], flat[:, 8:12], flat[:, 12:60]
    else:
        pos, so, rot, sh = verts["position"][:, :3], verts["scale_opacity"], verts["rotation"], verts["sh"]
    sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 16, 3)
    if sh16:
        sh = sh.astype(np.float16).astype(np.float32)
    return (np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(so[:, :3], np.float32), np.ascontiguousarray(rot, np.float32),
            np.ascontiguousarray(so[:, 3], np.float32), sh)


def clamp_branches(pos, uniforms):
    """The binary32 restatement of gs_preprocess.hip's p_view rows and its one division per axis.  Returns (p_view [n][3] float32,
    ratio [n][2] float32 = tx/tz ty/tz, clamped [n][2] float32 = fminf(lim, fmaxf(-lim, ratio)), lim [2] float32); the clamp binds
    where clamped != ratio, and `clamped` is then the constant the frame multiplied tz with."""
    vm = np.asarray(uniforms["view_mat"], _F).reshape(16)
    p = np.asarray(pos, _F)
    rows = []
    for r in range(3):
        s = vm[0 * 4 + r] * p[:, 0]
        s = s + vm[1 * 4 + r] * p[:, 1]
        s = s + vm[2 * 4 + r] * p[:, 2]
        s = s + vm[3 * 4 + r] * _F(1.0)
        rows.append(s)
    pv = np.stack(rows, axis=1)
    lim = np.array([_F(1.3) * _F(np.asarray(uniforms["tan_fovx"]).reshape(-1)[0]), _F(1.3) * _F(np.asarray(uniforms["tan_fovy"]).reshape(-1)[0])], _F)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.stack([pv[:, 0] / pv[:, 2], pv[:, 1] / pv[:, 2]], axis=1).astype(_F)
        clamped = np.minimum(lim[None, :], np.maximum(-lim[None, :], ratio)).astype(_F)
    return pv, ratio, clamped, lim


def sh_basis(x, y, z):
    """The sixteen basis values of sh_to_rgb (signs and constants included, the 0.5 not) and their partials with respect to x, y, z,
    as polynomials in three independent variables: [(B, dB/dx, dB/dy, dB/dz)] * 16 of V (a python 0.0 where a partial vanishes)."""
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    c2, c3 = SH_C2, SH_C3
    one = V(np.ones_like(x.v))
    b = [(one * SH_C0, 0.0, 0.0, 0.0),
         (y * -SH_C1, 0.0, one * -SH_C1, 0.0),
         (z * SH_C1, 0.0, 0.0, one * SH_C1),
         (x * -SH_C1, one * -SH_C1, 0.0, 0.0),
         (xy * c2[0], y * c2[0], x * c2[0], 0.0),
         (yz * c2[1], 0.0, z * c2[1], y * c2[1]),
         ((zz.pow2(1) - xx - yy) * c2[2], (x * c2[2]).pow2(1).__neg__(), (y * c2[2]).pow2(1).__neg__(), (z * c2[2]).pow2(2)),
         (xz * c2[3], z * c2[3], 0.0, x * c2[3]),
         ((xx - yy) * c2[4], (x * c2[4]).pow2(1), (y * c2[4]).pow2(1).__neg__(), 0.0),
         ((xx * 3.0 - yy) * y * c3[0], xy * (6.0 * c3[0]), (xx * 3.0 - yy * 3.0) * c3[0], 0.0),
         (xy * z * c3[1], yz * c3[1], xz * c3[1], xy * c3[1]),
         ((zz.pow2(2) - xx - yy) * y * c3[2], (xy * c3[2]).pow2(1).__neg__(), (zz.pow2(2) - xx - yy * 3.0) * c3[2], (yz * c3[2]).pow2(3)),
         (z * (zz.pow2(1) - xx * 3.0 - yy * 3.0) * c3[3], xz * (-6.0 * c3[3]), yz * (-6.0 * c3[3]), (zz * 6.0 - xx * 3.0 - yy * 3.0) * c3[3]),
         (x * (zz.pow2(2) - xx - yy) * c3[4], (zz.pow2(2) - xx * 3.0 - yy) * c3[4], (xy * c3[4]).pow2(1).__neg__(), (xz * c3[4]).pow2(3)),
         ((xx - yy) * z * c3[5], (xz * c3[5]).pow2(1), (yz * c3[5]).pow2(1).__neg__(), (xx - yy) * c3[5]),
         (x * (xx - yy * 3.0) * c3[6], (xx * 3.0 - yy * 3.0) * c3[6], xy * (-6.0 * c3[6]), 0.0)]
    return b


def backward(pos, scale, quat, opacity, sh, uniforms, visible, red_flows, colour=None, opacity_grad=None, conic=None, uv=None,
             antialiased=False, sh_rest_coeffs=15, mutate=None):
    """pos [n][3], scale [n][3], quat [n][4], opacity [n], sh [n][16][3]: the stored binary32 values.  uniforms: one gs_uniforms
    record.  visible, red_flows: bool [n], the frame's decisions.  colour [n][3], opacity_grad [n], conic [n][3], uv [n][2]:
    float64 input gradients, None = zeros.  Returns dict(means, log_scales, quats, opacity_logits, sh_dc, sh_rest: float64 sums of
    the shapes gs_project_grads documents (culled rows 0); A = {name: magnitudes}; k = {name: the counted roundings};
    visible; binds = bool [n][2]; det_raw = float64 [n] (NaN where culled); det_raw_bound = float64 [n], its counted roundings times
    2^-53 times its magnitude (how far a binary64 evaluation of det_raw may lie from the exact one; NaN where culled); margin = {"clamp": |tx/tz| / lim, "r": rgb0};
    record = {field of RECORD: (value [n][c], magnitude [n][c], counted roundings)}, the forward value of F (NaN where culled): uv,
    the conic's three numbers, the opacity after the antialiased factor, rgb before and after red's clamp -- each within
    count 2^-53 magnitude of exact, by the rules above."""
    assert mutate is None or mutate in MUTATIONS, mutate
    assert sh_rest_coeffs in (0, 3, 8, 15)
    n = len(pos)
    idx = np.nonzero(visible)[0]
    nv = len(idx)
    f64 = np.float64
    u = uniforms[0] if getattr(uniforms, "shape", ()) else uniforms
    pm, vm = np.asarray(u["proj_mat"], f64).reshape(16), np.asarray(u["view_mat"], f64).reshape(16)
    W, H = float(u["width"]), float(u["height"])
    tan_x, tan_y = float(_F(u["tan_fovx"])), float(_F(u["tan_fovy"]))
    cam = np.asarray(u["camera_position"], f64).reshape(-1)[:3]
    P = lambda r, c: float(pm[c * 4 + r])   # noqa: E731
    Vm = lambda r, c: float(vm[c * 4 + r])  # noqa: E731
    Vt = lambda r, c: float(vm[r * 4 + c])  # noqa: E731  (the transposed read of the mutations)
    V_a = Vt if mutate == "view_transposed_in_a" else Vm
    V_gj = Vt if mutate == "view_transposed_in_g_j" else Vm
    V_gp = Vt if mutate == "view_transposed" else Vm

    def g_in(a, shape):
        if a is None:
            return np.zeros((nv,) + shape)
        a = np.asarray(a, f64)
        assert a.shape == (n,) + shape, (a.shape, shape)
        return a[idx]
    g_rgb, g_op, g_con, g_uv = g_in(colour, (3,)), g_in(opacity_grad, ()), g_in(conic, (3,)), g_in(uv, (2,))

    _, ratio, clamped, _ = clamp_branches(pos, u)
    binds_all = clamped != ratio
    binds, cconst = binds_all[idx], clamped[idx].astype(f64)

    p = [V(pos[idx, c].astype(f64)) for c in range(3)]
    s = [V(scale[idx, c].astype(f64)) for c in range(3)]
    q = [V(quat[idx, c].astype(f64)) for c in range(4)]
    o = V(opacity[idx].astype(f64))
    shv = sh[idx].astype(f64)                                     # [nv][16][3]
    flows0 = np.ones(nv, bool) if mutate == "red_always_flows" else np.asarray(red_flows, bool)[idx]

    # ---- forward
    h = {r: _sum([p[0] * P(r, 0), p[1] * P(r, 1), p[2] * P(r, 2)]) + P(r, 3) for r in (0, 1, 3)}
    t = [_sum([p[0] * Vm(r, 0), p[1] * Vm(r, 1), p[2] * Vm(r, 2)]) + Vm(r, 3) for r in range(3)]
    fx, fy = V(W) / (2.0 * tan_x), V(H) / (2.0 * tan_y)
    t2sq = t[2] * t[2]
    # tx / t2^2 of J's third column: t_a / t2^2 where the clamp does not bind, c / t2 where it does
    j_a2 = [(-(f * t[a]) / t2sq).where(~binds[:, a], -(f * V(cconst[:, a])) / t[2]) for a, f in ((0, fx), (1, fy))]
    j_aa = [fx / t[2], fy / t[2]]
    # A = J V  (2 x 3)
    A = [[j_aa[i] * V_a(i, c) + j_a2[i] * V_a(2, c) for c in range(3)] for i in range(2)]
    nrm = _sum([q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]]).sqrt()
    qh = [qq / nrm for qq in q]
    w_, x_, y_, z_ = qh
    R = [[1.0 - (y_ * y_ + z_ * z_).pow2(1), (x_ * y_ - z_ * w_).pow2(1), (x_ * z_ + y_ * w_).pow2(1)],
         [(x_ * y_ + z_ * w_).pow2(1), 1.0 - (x_ * x_ + z_ * z_).pow2(1), (y_ * z_ - x_ * w_).pow2(1)],
         [(x_ * z_ - y_ * w_).pow2(1), (y_ * z_ + x_ * w_).pow2(1), 1.0 - (x_ * x_ + y_ * y_).pow2(1)]]
    M = [[_sum([A[i][c] * R[c][k] for c in range(3)]) for k in range(3)] for i in range(2)]
    s2 = [sk if mutate == "s_not_squared" else sk * sk for sk in s]
    cov00 = _sum([M[0][k] * M[0][k] * s2[k] for k in range(3)])
    cov01 = _sum([M[0][k] * M[1][k] * s2[k] for k in range(3)])
    cov11 = _sum([M[1][k] * M[1][k] * s2[k] for k in range(3)])
    m00, m11, m01 = cov00 + DILATION, cov11 + DILATION, cov01
    det = m00 * m11 - m01 * m01
    c00, c01, c11 = m11 / det, -m01 / det, m00 / det
    rec_uv = [((h[0] / h[3] + 1.0) * W - 1.0).pow2(-1), ((h[1] / h[3] + 1.0) * H - 1.0).pow2(-1)]
    rec_op = o

    # ---- backward: conic (and comp) -> cov
    gc00, gc01, gc11 = V(g_con[:, 0]), V(g_con[:, 1]), V(g_con[:, 2])
    g_det = -(_sum([gc00 * c00, gc01 * c01, gc11 * c11]) / det)
    g_o = V(g_op)
    g_detraw = None
    det_raw_full, det_raw_bound = np.full(n, np.nan), np.full(n, np.nan)
    if antialiased:
        det_raw = cov00 * cov11 - cov01 * cov01
        det_raw_full[idx], det_raw_bound[idx] = det_raw.v, det_raw.k * U53 * det_raw.m
        pos_raw = det_raw.v > 0.0
        safe = V(np.where(pos_raw, det_raw.v, 1.0), np.where(pos_raw, det_raw.m, 1.0), det_raw.k)
        comp = (safe / det).sqrt()
        g_comp = V(g_op) * o
        g_o = (V(g_op) * comp).where(pos_raw, 0.0)
        rec_op = (o * comp).where(pos_raw, 0.0)
        if mutate != "no_comp_cov":
            g_detraw = (g_comp.pow2(-1) / (comp * det)).where(pos_raw, 0.0)
            g_det = g_det + (-(g_comp * comp).pow2(-1) / det).where(pos_raw, 0.0)
    g_m00 = gc11 / det + g_det * m11
    g_m11 = gc00 / det + g_det * m00
    g_m01 = -(gc01 / det) - (g_det * m01).pow2(1)
    if g_detraw is not None:
        g_m00 = g_m00 + g_detraw * cov11
        g_m11 = g_m11 + g_detraw * cov00
        g_m01 = g_m01 - (g_detraw * cov01).pow2(1)
    # cov -> M, s^2
    g_M = [[(g_m00 * M[0][k]).pow2(1) + g_m01 * M[1][k] for k in range(3)], [(g_m11 * M[1][k]).pow2(1) + g_m01 * M[0][k] for k in range(3)]]
    g_M = [[g_M[i][k] * s2[k] for k in range(3)] for i in range(2)]
    g_s2 = [_sum([g_m00 * (M[0][k] * M[0][k]), g_m01 * (M[0][k] * M[1][k]), g_m11 * (M[1][k] * M[1][k])]) for k in range(3)]
    d_ls = [(g_s2[k] * s[k]) if mutate == "s_not_squared" else (g_s2[k] * s2[k]).pow2(1) for k in range(3)]
    # M = A R
    g_A = [[_sum([g_M[i][k] * R[c][k] for k in range(3)]) for c in range(3)] for i in range(2)]
    g_R = [[A[0][c] * g_M[0][k] + A[1][c] * g_M[1][k] for k in range(3)] for c in range(3)]
    # A = J V
    g_Jaa = [_sum([g_A[i][c] * V_gj(i, c) for c in range(3)]) for i in range(2)]
    g_Ja2 = [_sum([g_A[i][c] * V_gj(2, c) for c in range(3)]) for i in range(2)]
    # J -> t
    t2cu = t2sq * t[2]
    g_t = [None, None, None]
    g_t2_terms = []
    for a, f in ((0, fx), (1, fy)):
        g_t[a] = (-(g_Ja2[a] * f) / t2sq).where(~binds[:, a], 0.0)
        free = (g_Ja2[a] * f * t[a]).pow2(1) / t2cu
        if mutate == "clamp_is_constant":
            bound = (g_Ja2[a] * f * (V(cconst[:, a]) * t[2])).pow2(1) / t2cu
        else:
            bound = (g_Ja2[a] * f * V(cconst[:, a])) / t2sq
        g_t2_terms += [-(g_Jaa[a] * f) / t2sq, free.where(~binds[:, a], bound)]
    g_t[2] = _sum(g_t2_terms)
    g_p = [_sum([g_t[r] * V_gp(r, c) for r in range(3)]) for c in range(3)]
    # uv -> p
    h3sq = h[3] * h[3]
    for c in range(3):
        du = (P(0, c) / h[3] - (h[0] * P(3, c)) / h3sq) * (W / 2.0)
        dv = (P(1, c) / h[3] - (h[1] * P(3, c)) / h3sq) * (H / 2.0)
        g_p[c] = g_p[c] + V(g_uv[:, 0]) * du + V(g_uv[:, 1]) * dv
    # R -> q^ -> q
    gR = g_R
    g_qh = [(_sum([-(z_ * gR[0][1]), y_ * gR[0][2], z_ * gR[1][0], -(x_ * gR[1][2]), -(y_ * gR[2][0]), x_ * gR[2][1]])).pow2(1),
            (_sum([-(x_ * gR[1][1]).pow2(1), -(x_ * gR[2][2]).pow2(1), y_ * gR[0][1], z_ * gR[0][2], y_ * gR[1][0], -(w_ * gR[1][2]),
                   z_ * gR[2][0], w_ * gR[2][1]])).pow2(1),
            (_sum([-(y_ * gR[0][0]).pow2(1), -(y_ * gR[2][2]).pow2(1), x_ * gR[0][1], w_ * gR[0][2], x_ * gR[1][0], z_ * gR[1][2],
                   -(w_ * gR[2][0]), z_ * gR[2][1]])).pow2(1),
            (_sum([-(z_ * gR[0][0]).pow2(1), -(z_ * gR[1][1]).pow2(1), -(w_ * gR[0][1]), x_ * gR[0][2], w_ * gR[1][0], y_ * gR[1][2],
                   x_ * gR[2][0], y_ * gR[2][1]])).pow2(1)]
    if mutate == "no_tangent_projection":
        d_q = [g / nrm for g in g_qh]
    else:
        dot = _sum([qh[c] * g_qh[c] for c in range(4)])
        d_q = [(g_qh[c] - qh[c] * dot) / nrm for c in range(4)]
    # rgb -> sh, and -> d -> p
    rel = [p[c] - (0.0 if mutate == "camera_at_origin" else float(cam[c])) for c in range(3)]
    ln = _sum([rel[0] * rel[0], rel[1] * rel[1], rel[2] * rel[2]]).sqrt()
    d = [r / ln for r in rel]
    basis = sh_basis(*d)
    grgb = [V(g_rgb[:, 0]).where(flows0, 0.0), V(g_rgb[:, 1]), V(g_rgb[:, 2])]
    d_sh = [[basis[j][0] * grgb[k] for k in range(3)] for j in range(16)]
    if mutate != "no_direction":
        g_d = []
        for a in range(3):
            terms = []
            for j in range(1, 16):
                part = basis[j][1 + a]
                if isinstance(part, float):
                    continue
                S = _sum([V(shv[:, j, k]) * grgb[k] for k in range(3)])
                terms.append(part * S)
            g_d.append(_sum(terms))
        dg = _sum([d[a] * g_d[a] for a in range(3)])
        for c in range(3):
            g_p[c] = g_p[c] + (g_d[c] - d[c] * dg) / ln
    # opacity
    d_logit = g_o * (o * (1.0 - o))

    K = sh_rest_coeffs
    cols = dict(means=g_p, log_scales=d_ls, quats=d_q, opacity_logits=[d_logit], sh_dc=d_sh[0],
                sh_rest=[d_sh[j][k] for j in range(1, 1 + K) for k in range(3)])
    shapes = dict(means=(n, 3), log_scales=(n, 3), quats=(n, 4), opacity_logits=(n,), sh_dc=(n, 3), sh_rest=(n, K, 3))
    out, mags, counts = {}, {}, {}
    for name, vs in cols.items():
        val, mag = np.zeros((n, len(vs))), np.zeros((n, len(vs)))
        for c, v in enumerate(vs):
            val[idx, c], mag[idx, c] = v.v, v.m
        out[name], mags[name] = val.reshape(shapes[name]), mag.reshape(shapes[name])
        counts[name] = max([v.k for v in vs], default=0)
        assert counts[name] <= K_PATH, (name, counts[name])
    rgb_raw = [_sum([basis[j][0] * V(shv[:, j, k]) for j in range(16)]) + 0.5 for k in range(3)]
    rgb0 = np.full(n, np.nan)
    rgb0[idx] = rgb_raw[0].v
    fields = dict(uv=rec_uv, conic=[c00, c01, c11], opacity=[rec_op], rgb_raw=rgb_raw,
                  rgb=[rgb_raw[0].where(np.asarray(red_flows, bool)[idx], 0.0), rgb_raw[1], rgb_raw[2]])
    record = {}
    for name, vs in fields.items():
        val, mag = np.full((n, len(vs)), np.nan), np.full((n, len(vs)), np.nan)
        for c, v in enumerate(vs):
            val[idx, c], mag[idx, c] = v.v, v.m
        record[name] = (val, mag, max(v.k for v in vs))
    lim_ratio = np.full((n, 2), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        _, _, _, lim = clamp_branches(pos, u)
        lim_ratio[idx] = np.abs(ratio[idx].astype(f64)) / lim.astype(f64)[None, :]
    out.update(A=mags, k=counts, visible=np.asarray(visible, bool), binds=binds_all & np.asarray(visible, bool)[:, None],
               det_raw=det_raw_full, det_raw_bound=det_raw_bound, margin=dict(clamp=lim_ratio, r=rgb0), record=record)
    return out


def bound(want, name, preload=0.0, times=1):
    """The element-wise bound on |got - (preload + times * want[name])| after `times` calls into an array preloaded with `preload`
    (a scalar or an array of the output's shape)."""
    return 2.0 * times * ((K_PATH + times) * want["A"][name] + np.abs(np.asarray(preload, np.float64)) * (want["A"][name] > 0)) * U53
