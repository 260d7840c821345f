"""The yardstick of gs_blend_backward (include/gs3d_hip.h): the definition restated from the oracle's stage outputs.

A pixel walks its tile's list as render.comp:61-89 does, exactly as tests/lift_reference.py walks it: numpy binary32 with one
rounding per operation and the oracle's restatement of libm's expf; `power > 0` skips an entry, `alpha < 1/255` skips it,
`T (1 - alpha) < 1e-4` ends the walk.  The walk accumulates the image on the way (it must equal the oracle's bit for bit:
tests/test_blend_backward_api.py) and keeps, per blended (entry, pixel) pair, what the definition names: alpha_i, T_i (before :88),
e_i, prod_i = fl32(o e_i), dx_i, dy_i.  Then, in binary64 on exact conversions of those, with G = grad_rgb[p], ga = grad_alpha[p]
or 0, L_p the pixel's blended entries and T_f its final T:
    a_i = G_r r + G_g g + G_b b       w_i = float64(fl32(alpha_i T_i))       R_i = sum over j > i of a_j w_j   (a suffix sum here)
    colour[g]  += w_i G
    galpha_i    = T_i a_i - (R_i - ga T_f) / m_i,   m_i = fl32(1 - alpha_i)
    where prod_i <= 0.99 (the pair FLOWS: alpha is the product, not the clamp; false for a NaN product):
        opacity[g] += galpha_i e_i          gp = galpha_i alpha_i
        conic[g]   += gp (-0.5 dx^2, -dx dy, -0.5 dy^2)         uv[g] += gp (-(c00 dx + c01 dy), -(c01 dx + c11 dy))
colour is accumulated as lift_reference.lift accumulates `out` -- the same terms in the same order, so the two are equal bit for
bit; the other three are summed per (tile, entry) with numpy's sum and added in list order.

THE BOUND.  The definition leaves open the order of the adds and the association inside a term, so beside the sums the module
returns, per output, terms[name][g] = n_g, the number of terms Gaussian g receives (blended pairs for colour, flowing pairs for
the other three), and a magnitude A[name] in which every term enters with the absolute values of its constituents:
    mag(galpha_i) = T_i |a_i| + ((L_p + 2) M_p + |ga| T_f) / m_i,   |a_i| = |G_r r| + |G_g g| + |G_b b|,   M_p = sum_j |a_j| w_j
times the magnitude of the downstream factor (e_i; alpha_i (0.5 dx^2, |dx dy|, 0.5 dy^2); alpha_i (|c00 dx| + |c01 dy|, ..)),
and |w_i G| for colour.  With u = 2^-53, to first order, one term computed in binary64 in ANY association differs from its exact
value by at most 8 u times its magnitude:
  - the products G r, ga T_f, dx dx, dx dy, c dx of two binary32 values are exact; w_i is an exact conversion;
  - a_i: 2 adds, each within u |a_i|;  T_i a_i: 1 product;  the final subtraction of galpha_i: 1.  That is 4 on the T_i |a_i| part;
  - every summand a_j w_j of R_i: 2 (its a_j) + 1 (the product) = 3 u |a_j| w_j, once -- an implementation that forms R_i as a
    total minus a prefix must use the same summands in both, as gs_backward.hip does;
    R_i as a suffix sum: at most L_p - 1 adds, (L_p - 1) u M_p;  as a total (L_p - 1 adds) minus a prefix (i - 1 adds), one
    subtraction: at most (2 L_p - 1) u M_p.  With the 3 u M_p of the summands: at most (2 L_p + 2) u M_p = 2 u (L_p + 1) M_p --
    under 2 u times the (L_p + 2) M_p that R_i enters the magnitude with;
    R_i - ga T_f: 1;  the division by m_i: 1;  the final subtraction: 1.  That is 2 + 3 = 5 on the R part, and 3 on |ga| T_f / m_i;
  - downstream: galpha e: 1;  gp = galpha alpha: 1, times an exact factor: 1 more (conic: 2);  uv's factor is a rounded sum: 3.
So a term is within (5 + 3) u = 8 u of exact, relative to its magnitude, and the sum of n_g such terms in any order of binary64
adds within (n_g - 1) u A more: |computed - exact| <= (n_g + 7) u A, and with the second-order terms (n_g + 8) u A.  This module's
own sums obey the same bound, so for every element
    |got - want| <= 2 (n_g + k) 2^-53 A,    k = 8 = K_TERM
-- the factor 2 as in tests/test_gpu_lift.py: both sides lie within the bound of the exact sum.  A statement about binary64
arithmetic, not a measurement.  An element that held x before the call counts x as one more term: n_g + 1, A + |x|.

With dtype=np.float64 the same code walks in binary64 (exp = numpy's) and takes NO decision of its own: `replay` = the "pairs" of
the binary32 walk says which pixels blend each entry and which of those pairs flow, and alpha is 0.99 where a pair does not flow.
That variant is the exact derivative of a smooth function and is compared with torch.autograd (tests/test_blend_backward_api.py).

Vectorised over a tile's pixels, Python loops over the tile's entries.  A plain module: numpy and the oracle only."""
import numpy as np

K_TERM = 8
OUTPUTS = {"colour": 3, "opacity": 1, "conic": 3, "uv": 2}


def backward(oracle, ref, width, height, grad_rgb, grad_alpha=None, dtype=np.float32, replay=None):
    """ref: oracle.stages(...) of the frame.  grad_rgb (height, width, 3) float32, grad_alpha None or (height, width) float32.
    Returns dict(colour [N, 3], opacity [N], conic [N, 3], uv [N, 2] float64; terms = {name: int64 [N]}; A = {name: float64 of the
    output's shape}; image float32 [height, width, 4]; alpha float64 [height, width] = 1 - T_f; blended int32 [height, width] =
    L_p; broken bool [height, width] = the pixel's walk ended at :83; clamped = the number of blended pairs that do not flow;
    pairs = {tile: [(list position, pixels of the tile that blend it, which of them flow)]}, the decisions for `replay`)."""
    F = np.dtype(dtype).type
    exact = F is np.float32
    assert exact or replay is not None, "the binary64 walk replays the decisions of the binary32 walk"
    attr, bounds, payload = ref["attr"], ref["boundaries"].astype(np.int64), ref["sorted_payload"]
    n = len(attr)
    G_all = np.ascontiguousarray(grad_rgb, np.float32)
    assert G_all.shape == (height, width, 3)
    ga_all = np.zeros((height, width), np.float32) if grad_alpha is None else np.ascontiguousarray(grad_alpha, np.float32)
    assert ga_all.shape == (height, width)
    sums = {k: np.zeros((n, c) if c > 1 else (n,), np.float64) for k, c in OUTPUTS.items()}
    A = {k: np.zeros_like(v) for k, v in sums.items()}
    terms = {k: np.zeros(n, np.int64) for k in OUTPUTS}
    blended = np.zeros((height, width), np.int32)
    broken = np.zeros((height, width), bool)
    alpha_map = np.zeros((height, width), np.float64)
    image = np.zeros((height, width, 4), np.float32)
    image[..., 3] = 1.0
    pairs, clamped = {}, 0
    co_all, uv_all, col_all = attr["conic_opacity"].astype(F), attr["uv"].astype(F), attr["color_radii"].astype(F)
    tx, ty = (width + 15) // 16, (height + 15) // 16
    for t in range(tx * ty):
        x0, y0 = 16 * (t % tx), 16 * (t // tx)
        ys, xs = np.mgrid[y0:min(y0 + 16, height), x0:min(x0 + 16, width)]
        ys, xs = ys.ravel(), xs.ravel()
        fx, fy = xs.astype(F), ys.astype(F)
        G64 = G_all[ys, xs].astype(np.float64)
        ga64 = ga_all[ys, xs].astype(np.float64)
        npix = len(xs)
        T = np.ones(npix, F)
        walking = np.ones(npix, bool)
        c = np.zeros((npix, 3), F)
        nb = np.zeros(npix, np.int32)
        M = np.zeros(npix, np.float64)
        kept, decided = [], []     # per blended entry of the tile, front to back
        ids = payload[bounds[2 * t]:bounds[2 * t + 1]]
        given = {pos: (at, fl) for pos, at, fl in replay[t]} if replay is not None else None
        for pos, g in enumerate(ids):
            co, uv = co_all[g], uv_all[g]
            dx, dy = uv[0] - fx, uv[1] - fy
            power = F(-0.5) * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy            # :66
            if given is None:
                if not walking.any():
                    break
                with np.errstate(invalid="ignore"):
                    reach = walking & (power <= F(0.0))                                        # :68 (a NaN power skips the entry)
                if not reach.any():
                    continue
                at = np.nonzero(reach)[0]
                pw = power[at]
                ex = np.zeros(len(at), np.float32)
                fits = pw >= F(-103.0)               # (below: libm's expf is at most a denormal, alpha far below the cut)
                ex[fits] = oracle.expf_libm(pw[fits])
                prod = co[3] * ex
                with np.errstate(invalid="ignore"):
                    flows = prod <= F(0.99)                                                    # (false for a NaN product)
                alpha = np.where(flows, prod, F(0.99)).astype(np.float32)                      # :77 (min(0.99, NaN) = 0.99)
                keep = ~(alpha < F(1.0) / F(255.0))                                            # :78
                at, alpha, ex, flows = at[keep], alpha[keep], ex[keep], flows[keep]
                test_T = T[at] * (F(1.0) - alpha)
                brk = test_T < F(0.0001)                                                       # :82-85
                walking[at[brk]] = False
                at, alpha, ex, flows, test_T = at[~brk], alpha[~brk], ex[~brk], flows[~brk], test_T[~brk]
                if len(at) == 0:
                    continue
            else:
                if pos not in given:
                    continue
                at, flows = given[pos]
                ex = np.exp(power[at])
                alpha = np.where(flows, co[3] * ex, F(np.float32(0.99)))
                test_T = T[at] * (F(1.0) - alpha)
            Ti = T[at].copy()
            w64 = (alpha * Ti).astype(np.float64)                                              # fl(alpha T), T before :88
            c[at] = c[at] + (col_all[g][:3][None, :] * alpha[:, None]) * Ti[:, None]           # :87
            T[at] = test_T
            nb[at] += 1
            decided.append((pos, at, flows))
            # d_colour, accumulated as lift_reference.lift accumulates `out`
            prods = w64[:, None] * G64[at]                                                     # exact: 24 x 24 bits (binary32 walk)
            for row in prods:                                                                  # one binary64 add per term
                sums["colour"][g] += row
            A["colour"][g] += np.abs(prods).sum(axis=0)
            terms["colour"][g] += len(at)
            rgb = col_all[g][:3].astype(np.float64)
            a = (G64[at, 0] * rgb[0] + G64[at, 1] * rgb[1]) + G64[at, 2] * rgb[2]
            a_abs = np.abs(G64[at, 0] * rgb[0]) + np.abs(G64[at, 1] * rgb[1]) + np.abs(G64[at, 2] * rgb[2])
            M[at] += a_abs * w64
            kept.append((g, at, flows, alpha.astype(np.float64), Ti.astype(np.float64), ex.astype(np.float64),
                         (F(1.0) - alpha).astype(np.float64), dx[at].astype(np.float64), dy[at].astype(np.float64), a, a_abs, a * w64))
        Tf = T.astype(np.float64)
        suffix = np.zeros(npix, np.float64)                                                    # R_i: what lies behind entry i
        for g, at, flows, alpha, Ti, ex, m, dxd, dyd, a, a_abs, aw in reversed(kept):
            R = suffix[at]
            suffix[at] = suffix[at] + aw
            clamped += int((~flows).sum())
            if not flows.any():
                continue
            f = flows
            galpha = (Ti * a - (R - ga64[at] * Tf[at]) / m)[f]
            mag = (Ti * a_abs + ((nb[at] + 2.0) * M[at] + np.abs(ga64[at]) * Tf[at]) / m)[f]
            alpha, ex, dxd, dyd = alpha[f], ex[f], dxd[f], dyd[f]
            gp, magp = galpha * alpha, mag * np.abs(alpha)
            c00, c01, c11 = (float(v) for v in co_all[g][:3])
            sums["opacity"][g] += (galpha * ex).sum()
            A["opacity"][g] += (mag * np.abs(ex)).sum()
            conic = np.stack([-0.5 * (dxd * dxd), -(dxd * dyd), -0.5 * (dyd * dyd)], axis=1)
            sums["conic"][g] += (gp[:, None] * conic).sum(axis=0)
            A["conic"][g] += (magp[:, None] * np.abs(conic)).sum(axis=0)
            uvf = np.stack([-(c00 * dxd + c01 * dyd), -(c01 * dxd + c11 * dyd)], axis=1)
            uvm = np.stack([np.abs(c00 * dxd) + np.abs(c01 * dyd), np.abs(c01 * dxd) + np.abs(c11 * dyd)], axis=1)
            sums["uv"][g] += (gp[:, None] * uvf).sum(axis=0)
            A["uv"][g] += (magp[:, None] * uvm).sum(axis=0)
            for k in ("opacity", "conic", "uv"):
                terms[k][g] += int(f.sum())
        image[ys, xs, :3] = c
        blended[ys, xs] = nb
        broken[ys, xs] = ~walking
        alpha_map[ys, xs] = 1.0 - Tf
        pairs[t] = decided
    return dict(sums, terms=terms, A=A, image=image, alpha=alpha_map, blended=blended, broken=broken, clamped=clamped, pairs=pairs)


def bound(want, name, preload=0.0, times=1):
    """2 (n_g + k) 2^-53 A for output `name`, as an array of the output's shape: after `times` calls into an array that held
    `preload` (one more term when it is not zero)."""
    n = want["terms"][name]
    n = n if want[name].ndim == 1 else n[:, None]
    return 2.0 * (times * n + K_TERM + (1 if preload != 0.0 else 0)) * 2.0 ** -53 * (times * want["A"][name] + abs(preload))
