"""The yardstick of gs_lift_pixels (include/gs3d_hip.h): the definition restated from the oracle's stage outputs.

A pixel walks its tile's list as render.comp:61-89 does, in numpy binary32 with one rounding per operation and the oracle's
restatement of libm's expf: `power > 0` skips an entry, `alpha < 1/255` skips it, `T (1 - alpha) < 1e-4` ends the walk.  An entry
of Gaussian g that reaches :87 at a counted pixel p (mask None or != 0 there) is blended with w = fl32(alpha T), T before :88, and
    out[g][c] += float64(w) * float64(values[p][c])        weight[g] += float64(w)
The products are exact in binary64; the sums are accumulated in binary64 in this module's own order (tile by tile, entry by
entry, pixel by pixel).  The definition leaves the order open, so beside the sums the module returns what bounds any order:
terms[g] = n_g, the number of terms Gaussian g receives, and A[g][c] = the sum of |w * values[p][c]| (abs_weight[g] for the
weights): every order of binary64 adds lies within (n_g - 1) 2^-53 A of the exact sum.

The walk accumulates the image on the way (`c += (colour * alpha) * T`, in that order): it must equal the oracle's image bit for
bit, which pins this module to the reference's arithmetic (tests/test_lift_api.py).

Vectorised over a tile's pixels, a Python loop over the tile's entries.  A plain module: numpy and the oracle only."""
import numpy as np

_F = np.float32


def lift(oracle, ref, width, height, values=None, mask=None):
    """ref: oracle.stages(...) of the frame.  values: None or (height, width, C) float32.  mask: None or (height, width),
    nonzero = counted.  Returns dict(out float64 [N, C] (C = 0 without values), weight float64 [N], terms int64 [N],
    A float64 [N, C], abs_weight float64 [N] (= weight: every w is > 0), blended int32 [height, width] = the entries blended at
    each pixel whether it is counted or not, image float32 [height, width, 4])."""
    attr, bounds, payload = ref["attr"], ref["boundaries"].astype(np.int64), ref["sorted_payload"]
    n = len(attr)
    vals = np.zeros((height, width, 0), np.float32) if values is None else np.ascontiguousarray(values, np.float32)
    assert vals.shape[:2] == (height, width)
    nc = vals.shape[2]
    out, A = np.zeros((n, nc), np.float64), np.zeros((n, nc), np.float64)
    weight, terms = np.zeros(n, np.float64), np.zeros(n, np.int64)
    blended = np.zeros((height, width), np.int32)
    image = np.zeros((height, width, 4), np.float32)
    image[..., 3] = 1.0
    counted_all = np.ones((height, width), bool) if mask is None else np.asarray(mask).reshape(height, width) != 0
    co_all, uv_all, col_all = attr["conic_opacity"], attr["uv"], attr["color_radii"]
    tx, ty = (width + 15) // 16, (height + 15) // 16
    for t in range(tx * ty):
        x0, y0 = 16 * (t % tx), 16 * (t // tx)
        ys, xs = np.mgrid[y0:min(y0 + 16, height), x0:min(x0 + 16, width)]
        ys, xs = ys.ravel(), xs.ravel()
        fx, fy = xs.astype(np.float32), ys.astype(np.float32)
        counted = counted_all[ys, xs]
        v64 = vals[ys, xs].astype(np.float64)
        npix = len(xs)
        T = np.ones(npix, np.float32)
        walking = np.ones(npix, bool)
        c = np.zeros((npix, 3), np.float32)
        nb = np.zeros(npix, np.int32)
        for g in payload[bounds[2 * t]:bounds[2 * t + 1]]:
            if not walking.any():
                break
            co, uv = co_all[g], uv_all[g]
            dx, dy = uv[0] - fx, uv[1] - fy
            power = _F(-0.5) * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy          # :66
            with np.errstate(invalid="ignore"):
                reach = walking & (power <= _F(0.0))                                          # :68 (a NaN power skips the entry)
            if not reach.any():
                continue
            at = np.nonzero(reach)[0]
            pw = power[at]
            ex = np.zeros(len(at), np.float32)
            fits = pw >= _F(-103.0)                  # (below: libm's expf is at most a denormal, alpha far below the cut)
            ex[fits] = oracle.expf_libm(pw[fits])
            prod = co[3] * ex
            alpha = np.where(np.isnan(prod), _F(0.99), np.minimum(_F(0.99), prod)).astype(np.float32)   # :77 (min(0.99, NaN) = 0.99)
            keep = ~(alpha < _F(1.0) / _F(255.0))                                             # :78
            at, alpha = at[keep], alpha[keep]
            test_T = T[at] * (_F(1.0) - alpha)
            brk = test_T < _F(0.0001)                                                         # :82-85
            walking[at[brk]] = False
            at, alpha, test_T = at[~brk], alpha[~brk], test_T[~brk]
            if len(at) == 0:
                continue
            w = alpha * T[at]                                                                 # fl32(alpha T), T before :88
            c[at] = c[at] + (col_all[g][:3][None, :] * alpha[:, None]) * T[at][:, None]       # :87
            T[at] = test_T
            nb[at] += 1
            cnt = counted[at]
            if not cnt.any():
                continue
            w64 = w[cnt].astype(np.float64)
            prods = w64[:, None] * v64[at[cnt]]                                               # exact: 24 x 24 bits
            for row in prods:                                                                 # one binary64 add per term
                out[g] += row
            A[g] += np.abs(prods).sum(axis=0)
            for x in w64:
                weight[g] += x
            terms[g] += int(cnt.sum())
        image[ys, xs, :3] = c
        blended[ys, xs] = nb
    return dict(out=out, weight=weight, terms=terms, A=A, abs_weight=weight.copy(), blended=blended, image=image)
