"""The yardstick of gs_camera_backward (include/gs3d_hip.h): the definition restated in numpy binary64.

THE FUNCTION is the record function F of gs_project_backward with the same branches as constants (visibility, each clamp's branch
as the binary32 restatement of k_preprocess takes it, red's flow by the record, det_raw <= 0 in an antialiased frame),
differentiated with respect to the frame's uniforms: V[r][c] = view_mat[4 c + r] rows 0..2 (through t = V (p, 1) and through
A = J V(3 x 3)), P[r][c] = proj_mat[4 c + r] rows 0, 1, 3 (through h = P (p, 1) to u v), camera_position (through the view
direction to rgb).  Row 3 of V and row 2 of P are not read by F.  The intrinsics carry no gradient.  Per visible Gaussian i the
chain runs to the nodes g_t, gA, g_h, g_d exactly as tests/project_backward_reference.py runs it (its class V, its clamp_branches,
its sh_basis and its unpacking are imported; the chain is restated here because that module returns none of its nodes), and the
27 terms are
    dV[r][c] = g_t[r] (p, 1)[c] + (r < 2 ? jaa[r] gA[r][c] : ja2[0] gA[0][c] + ja2[1] gA[1][c])   c < 3;     dV[r][3] = g_t[r]
    dP[r][c] = g_h[r] (p, 1)[c]
    dc       = -(g_d - d (d . g_d)) / |p - c|
The result is their sum over the visible Gaussians: here the EXACT sum of the binary64 terms, math.fsum.

THE BOUND has two counted constants.
  K_PATH  Every term is a triple (value, magnitude A_i, count) under the rules of tests/project_backward_reference.py, so a
          term computed in binary64 in any association is within  k 2^-53 A_i  of its exact value, the condition factors of h3,
          t2, the cov2D entries, det, det_raw and |p - c| carried in A_i.  k is counted by the arithmetic on the longest path: 647
          for an element of dV in an antialiased frame (g_t[2] of the Jacobian's third column times a position), 59 for dc, 18
          for dP; K_PATH = 650 bounds them all (asserted on every call).
  C_SUM   The device adds n = n_visible terms (zeros of culled lanes are exact) in some fixed tree: n - 1 roundings, each of a
          partial sum of magnitude at most S = sum_i A_i; then ONE add into the caller's array, of a content of at most |x| + S.
          C_SUM = 1:  (n - 1) + 1 + 1, the last one the single rounding of this module's own fsum.
Both sides' terms lie within K_PATH 2^-53 A_i of exact, so for every element, with S = sum_i A_i and x what the array held,
    |got - (x + want)| <= (2 K_PATH + n_visible + C_SUM) 2^-53 S + 2^-53 |x|
to first order.  A statement about arithmetic, not a fitted tolerance.  Where S is 0 the element keeps its bits (an exact zero
is not added); so do row 3 of view_mat and row 2 of proj_mat always.

`mutate` names single-term mutations; tests/test_camera_backward_api.py shows each fails against torch.autograd.
A plain module: numpy only."""
import math

import numpy as np

import project_backward_reference as pref
from project_backward_reference import V, _sum

U53 = pref.U53
K_PATH = 650
C_SUM = 1
OUTPUTS = {"view_mat": 16, "proj_mat": 16, "camera_position": 3}
MUTATIONS = ("no_a_term", "no_column_3", "clamp_not_binding", "camera_position_sign", "proj_row_2")
UNTOUCHED = {"view_mat": (3, 7, 11, 15), "proj_mat": (2, 6, 10, 14), "camera_position": ()}   # row 3 of V, row 2 of P: never written


def backward(pos, scale, quat, opacity, sh, uniforms, visible, red_flows, colour=None, opacity_grad=None, conic=None, uv=None,
             antialiased=False, mutate=None):
    """Arguments as project_backward_reference.backward.  Returns dict(view_mat [16], proj_mat [16] laid out as the uniforms'
    matrices, camera_position [3]: the exact sums of the per-Gaussian binary64 terms; A = {name: S, the summed magnitudes};
    terms = {name: [nv][elements]} and term_A likewise (the per-Gaussian terms and magnitudes, rows in the order of the visible
    ids); k = {name: counted roundings}; n_visible; visible; binds [n][2])."""
    assert mutate is None or mutate in MUTATIONS, mutate
    n = len(pos)
    idx = np.nonzero(visible)[0]
    nv = len(idx)
    f64 = np.float64
    u = uniforms[0] if getattr(uniforms, "shape", ()) else uniforms
    pm, vm = np.asarray(u["proj_mat"], f64).reshape(16), np.asarray(u["view_mat"], f64).reshape(16)
    W, H = float(u["width"]), float(u["height"])
    tan_x, tan_y = float(np.float32(u["tan_fovx"])), float(np.float32(u["tan_fovy"]))
    cam = np.asarray(u["camera_position"], f64).reshape(-1)[:3]
    P = lambda r, c: float(pm[c * 4 + r])   # noqa: E731
    Vm = lambda r, c: float(vm[c * 4 + r])  # noqa: E731

    def g_in(a, shape):
        if a is None:
            return np.zeros((nv,) + shape)
        a = np.asarray(a, f64)
        assert a.shape == (n,) + shape, (a.shape, shape)
        return a[idx]
    g_rgb, g_op, g_con, g_uv = g_in(colour, (3,)), g_in(opacity_grad, ()), g_in(conic, (3,)), g_in(uv, (2,))

    _, ratio, clamped, _ = pref.clamp_branches(pos, u)
    binds_all = clamped != ratio
    binds, cconst = binds_all[idx], clamped[idx].astype(f64)
    if mutate == "clamp_not_binding":
        binds = np.zeros_like(binds)

    p = [V(pos[idx, c].astype(f64)) for c in range(3)]
    s = [V(scale[idx, c].astype(f64)) for c in range(3)]
    q = [V(quat[idx, c].astype(f64)) for c in range(4)]
    o = V(opacity[idx].astype(f64))
    shv = sh[idx].astype(f64)
    flows0 = np.asarray(red_flows, bool)[idx]

    # ---- forward (project_backward_reference.backward, node for node)
    h = {r: _sum([p[0] * P(r, 0), p[1] * P(r, 1), p[2] * P(r, 2)]) + P(r, 3) for r in (0, 1, 3)}
    t = [_sum([p[0] * Vm(r, 0), p[1] * Vm(r, 1), p[2] * Vm(r, 2)]) + Vm(r, 3) for r in range(3)]
    fx, fy = V(W) / (2.0 * tan_x), V(H) / (2.0 * tan_y)
    t2sq = t[2] * t[2]
    j_a2 = [(-(f * t[a]) / t2sq).where(~binds[:, a], -(f * V(cconst[:, a])) / t[2]) for a, f in ((0, fx), (1, fy))]
    j_aa = [fx / t[2], fy / t[2]]
    A = [[j_aa[i] * Vm(i, c) + j_a2[i] * Vm(2, c) for c in range(3)] for i in range(2)]
    nrm = _sum([q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]]).sqrt()
    w_, x_, y_, z_ = [qq / nrm for qq in q]
    R = [[1.0 - (y_ * y_ + z_ * z_).pow2(1), (x_ * y_ - z_ * w_).pow2(1), (x_ * z_ + y_ * w_).pow2(1)],
         [(x_ * y_ + z_ * w_).pow2(1), 1.0 - (x_ * x_ + z_ * z_).pow2(1), (y_ * z_ - x_ * w_).pow2(1)],
         [(x_ * z_ - y_ * w_).pow2(1), (y_ * z_ + x_ * w_).pow2(1), 1.0 - (x_ * x_ + y_ * y_).pow2(1)]]
    M = [[_sum([A[i][c] * R[c][k] for c in range(3)]) for k in range(3)] for i in range(2)]
    s2 = [sk * sk for sk in s]
    cov00 = _sum([M[0][k] * M[0][k] * s2[k] for k in range(3)])
    cov01 = _sum([M[0][k] * M[1][k] * s2[k] for k in range(3)])
    cov11 = _sum([M[1][k] * M[1][k] * s2[k] for k in range(3)])
    m00, m11, m01 = cov00 + pref.DILATION, cov11 + pref.DILATION, cov01
    det = m00 * m11 - m01 * m01
    c00, c01, c11 = m11 / det, -m01 / det, m00 / det

    # ---- conic (and comp) -> cov -> M -> A
    gc00, gc01, gc11 = V(g_con[:, 0]), V(g_con[:, 1]), V(g_con[:, 2])
    g_det = -(_sum([gc00 * c00, gc01 * c01, gc11 * c11]) / det)
    g_detraw = None
    if antialiased:
        det_raw = cov00 * cov11 - cov01 * cov01
        pos_raw = det_raw.v > 0.0
        safe = V(np.where(pos_raw, det_raw.v, 1.0), np.where(pos_raw, det_raw.m, 1.0), det_raw.k)
        comp = (safe / det).sqrt()
        g_comp = V(g_op) * o
        g_detraw = (g_comp.pow2(-1) / (comp * det)).where(pos_raw, 0.0)
        g_det = g_det + (-(g_comp * comp).pow2(-1) / det).where(pos_raw, 0.0)
    g_m00 = gc11 / det + g_det * m11
    g_m11 = gc00 / det + g_det * m00
    g_m01 = -(gc01 / det) - (g_det * m01).pow2(1)
    if g_detraw is not None:
        g_m00 = g_m00 + g_detraw * cov11
        g_m11 = g_m11 + g_detraw * cov00
        g_m01 = g_m01 - (g_detraw * cov01).pow2(1)
    g_M = [[(g_m00 * M[0][k]).pow2(1) + g_m01 * M[1][k] for k in range(3)], [(g_m11 * M[1][k]).pow2(1) + g_m01 * M[0][k] for k in range(3)]]
    g_M = [[g_M[i][k] * s2[k] for k in range(3)] for i in range(2)]
    g_A = [[_sum([g_M[i][k] * R[c][k] for k in range(3)]) for c in range(3)] for i in range(2)]
    # ---- A = J V -> J -> t
    g_Jaa = [_sum([g_A[i][c] * Vm(i, c) for c in range(3)]) for i in range(2)]
    g_Ja2 = [_sum([g_A[i][c] * Vm(2, c) for c in range(3)]) for i in range(2)]
    t2cu = t2sq * t[2]
    g_t = [None, None, None]
    g_t2_terms = []
    for a, f in ((0, fx), (1, fy)):
        g_t[a] = (-(g_Ja2[a] * f) / t2sq).where(~binds[:, a], 0.0)
        free = (g_Ja2[a] * f * t[a]).pow2(1) / t2cu
        bound_ = (g_Ja2[a] * f * V(cconst[:, a])) / t2sq
        g_t2_terms += [-(g_Jaa[a] * f) / t2sq, free.where(~binds[:, a], bound_)]
    g_t[2] = _sum(g_t2_terms)
    # ---- uv -> h
    h3sq = h[3] * h[3]
    gu, gv = V(g_uv[:, 0]) * (W / 2.0), V(g_uv[:, 1]) * (H / 2.0)
    g_h = {0: gu / h[3], 1: gv / h[3], 3: -((gu * h[0] + gv * h[1]) / h3sq)}
    # ---- rgb -> d
    rel = [p[c] - float(cam[c]) for c in range(3)]
    ln = _sum([rel[0] * rel[0], rel[1] * rel[1], rel[2] * rel[2]]).sqrt()
    d = [r / ln for r in rel]
    basis = pref.sh_basis(*d)
    grgb = [V(g_rgb[:, 0]).where(flows0, 0.0), V(g_rgb[:, 1]), V(g_rgb[:, 2])]
    g_d = []
    for a in range(3):
        terms = []
        for j in range(1, 16):
            part = basis[j][1 + a]
            if isinstance(part, float):
                continue
            terms.append(part * _sum([V(shv[:, j, k]) * grgb[k] for k in range(3)]))
        g_d.append(_sum(terms))
    dg = _sum([d[a] * g_d[a] for a in range(3)])

    # ---- the 27 terms
    zero = V(np.zeros(nv))
    one = [p[0], p[1], p[2]]
    dV = {}
    for r in range(3):
        for c in range(3):
            through_t = g_t[r] * one[c]
            if mutate == "no_a_term":
                dV[r, c] = through_t
            elif r < 2:
                dV[r, c] = through_t + j_aa[r] * g_A[r][c]
            else:
                dV[r, c] = through_t + (j_a2[0] * g_A[0][c] + j_a2[1] * g_A[1][c])
        dV[r, 3] = zero if mutate == "no_column_3" else g_t[r]
    dP = {}
    for r in (0, 1, 3):
        for c in range(3):
            dP[r, c] = g_h[r] * one[c]
        dP[r, 3] = zero if mutate == "no_column_3" else g_h[r]
    if mutate == "proj_row_2":      # as if F read h2 the way it reads h3
        for c in range(4):
            dP[2, c] = dP[3, c]
    dc = [-((g_d[c] - d[c] * dg) / ln) for c in range(3)]
    if mutate == "camera_position_sign":
        dc = [-v for v in dc]

    cols = {"view_mat": {c * 4 + r: v for (r, c), v in dV.items()}, "proj_mat": {c * 4 + r: v for (r, c), v in dP.items()},
            "camera_position": dict(enumerate(dc))}
    out, mags, counts, terms, term_A = {}, {}, {}, {}, {}
    for name, size in OUTPUTS.items():
        val, mag = np.zeros(size), np.zeros(size)
        tv, tm = np.zeros((nv, size)), np.zeros((nv, size))
        k = 0
        for e, v in cols[name].items():
            tv[:, e], tm[:, e] = v.v, v.m
            val[e], mag[e] = math.fsum(v.v.tolist()), math.fsum(v.m.tolist())
            k = max(k, v.k)
        assert k <= K_PATH, (name, k)
        out[name], mags[name], counts[name], terms[name], term_A[name] = val, mag, k, tv, tm
    out.update(A=mags, k=counts, terms=terms, term_A=term_A, n_visible=nv, visible=np.asarray(visible, bool),
               binds=binds_all & np.asarray(visible, bool)[:, None])
    return out


def bound(want, name, preload=0.0, times=1):
    """The element-wise bound on |got - (preload + times * want[name])| after `times` calls into an array preloaded with `preload`."""
    S = want["A"][name]
    x = np.abs(np.asarray(preload, np.float64)) * (S > 0)
    return times * ((2.0 * K_PATH + want["n_visible"] + C_SUM) * S + x + (times - 1) * S) * U53
