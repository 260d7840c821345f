"""The yardstick of gs_accumulate_contributions (include/gs3d_hip.h): the definition restated from the oracle's stage outputs.

A pixel walks its tile's list as render.comp:61-89 does, in numpy binary32 with one rounding per operation and the oracle's
restatement of libm's expf: `power > 0` skips an entry, `alpha < 1/255` skips it, `T (1 - alpha) < 1e-4` ends the walk.  An entry
that reaches :87 is blended at that pixel with w = fl32(alpha T) and q = w 2^24 rounded to the nearest integer, ties to even.
Per Gaussian: weight = the sum of q, pixels = the count, over the counted pixels (mask != 0); per pixel: top_id = the id of the
largest w, the earlier entry on equal w, 0xFFFFFFFF where nothing was blended or the pixel is not counted.

The walk accumulates the image on the way (`c += (colour * alpha) * T`, in that order): it must equal the oracle's image bit for
bit, which pins this module to the reference's arithmetic (tests/test_contributions_api.py).

Vectorised over a tile's pixels, a Python loop over the tile's entries.  A plain module: numpy and the oracle only."""
import numpy as np

NONE = np.uint32(0xFFFFFFFF)
_F = np.float32


def contributions(oracle, ref, width, height, mask=None):
    """ref: oracle.stages(...) of the frame.  mask: None or (height, width), nonzero = counted.
    Returns dict(weight uint64 [N], pixels uint32 [N], top_id uint32 [height, width], image float32 [height, width, 4],
    blended = the number of counted (pixel, entry) pairs that reached :87)."""
    attr, bounds, payload = ref["attr"], ref["boundaries"].astype(np.int64), ref["sorted_payload"]
    n = len(attr)
    weight, pixels = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    top_id = np.full((height, width), NONE, np.uint32)
    image = np.zeros((height, width, 4), np.float32)
    image[..., 3] = 1.0
    counted_all = np.ones((height, width), bool) if mask is None else np.asarray(mask).reshape(height, width) != 0
    co_all, uv_all, col_all = attr["conic_opacity"], attr["uv"], attr["color_radii"]
    tx, ty = (width + 15) // 16, (height + 15) // 16
    blended = 0
    for t in range(tx * ty):
        x0, y0 = 16 * (t % tx), 16 * (t // tx)
        ys, xs = np.mgrid[y0:min(y0 + 16, height), x0:min(x0 + 16, width)]
        ys, xs = ys.ravel(), xs.ravel()
        fx, fy = xs.astype(np.float32), ys.astype(np.float32)
        counted = counted_all[ys, xs]
        npix = len(xs)
        T = np.ones(npix, np.float32)
        walking = np.ones(npix, bool)
        c = np.zeros((npix, 3), np.float32)
        best_w = np.zeros(npix, np.float32)          # every blended w is > 0
        best = np.full(npix, NONE, np.uint32)
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
            cnt = counted[at]
            q = np.rint(w[cnt].astype(np.float64) * 16777216.0).astype(np.uint64)             # exact product, ties to even
            weight[g] += q.sum(dtype=np.uint64)
            pixels[g] += np.uint32(cnt.sum())
            blended += int(cnt.sum())
            better = cnt & (w > best_w[at])          # strictly: the earlier entry stays on equal w
            best_w[at[better]] = w[better]
            best[at[better]] = g
        image[ys, xs, :3] = c
        top_id[ys, xs] = np.where(counted, best, NONE)
    return dict(weight=weight, pixels=pixels, top_id=top_id, image=image, blended=blended)
