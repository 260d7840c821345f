"""The yardstick of gs_blend_features (include/gs3d_hip.h): the definition restated from the oracle's stage outputs.

A pixel walks its tile's list as render.comp:61-89 does, in numpy binary32 with one rounding per operation and the oracle's
restatement of libm's expf: `power > 0` skips an entry, `alpha < 1/255` skips it, `T (1 - alpha) < 1e-4` ends the walk.  An entry
of Gaussian g that reaches :87 adds, with that line's alpha and T (T before :88),
    F[c] = F[c] + (features[g][c] * alpha) * T        D = D + (depth[g] * alpha) * T        (the order of :87)
    M    = depth[g]  if M is still unset and T * (1 - alpha) < 0.5
and at the walk's end the pixel gets features = F, depth = D, alpha = fl32(1 - T), median = M or +inf.  depth[g] is the
view-space depth of the frame's record, ref["attr"]["depth"].

With features = the records' colours the walk accumulates the image: it must equal the oracle's bit for bit, which pins this
module to the reference's arithmetic (tests/test_feature_maps_api.py).

Vectorised over a tile's pixels, a Python loop over the tile's entries.  A plain module: numpy and the oracle only."""
import numpy as np

_F = np.float32


def feature_maps(oracle, ref, width, height, features=None):
    """ref: oracle.stages(...) of the frame.  features: None or (N, C) float32.
    Returns dict(features float32 [height, width, C] (C = 0 without features), alpha, depth, median, T float32 [height, width])."""
    attr, bounds, payload = ref["attr"], ref["boundaries"].astype(np.int64), ref["sorted_payload"]
    feats = np.zeros((len(attr), 0), np.float32) if features is None else np.ascontiguousarray(features, np.float32)
    assert feats.shape[0] == len(attr)
    nc = feats.shape[1]
    out = np.zeros((height, width, nc), np.float32)
    alpha_map, depth_map = np.zeros((height, width), np.float32), np.zeros((height, width), np.float32)
    median_map = np.full((height, width), np.inf, np.float32)
    t_map = np.ones((height, width), np.float32)
    co_all, uv_all, dep_all = attr["conic_opacity"], attr["uv"], attr["depth"]
    tx, ty = (width + 15) // 16, (height + 15) // 16
    for t in range(tx * ty):
        x0, y0 = 16 * (t % tx), 16 * (t // tx)
        ys, xs = np.mgrid[y0:min(y0 + 16, height), x0:min(x0 + 16, width)]
        ys, xs = ys.ravel(), xs.ravel()
        fx, fy = xs.astype(np.float32), ys.astype(np.float32)
        npix = len(xs)
        T = np.ones(npix, np.float32)
        walking = np.ones(npix, bool)
        F = np.zeros((npix, nc), np.float32)
        D = np.zeros(npix, np.float32)
        M = np.full(npix, np.inf, np.float32)
        m_set = np.zeros(npix, bool)
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
            Tb = T[at]                                                                        # T before :88
            F[at] = F[at] + (feats[g][None, :] * alpha[:, None]) * Tb[:, None]                # :87
            D[at] = D[at] + (dep_all[g] * alpha) * Tb
            first = ~m_set[at] & (test_T < _F(0.5))
            M[at[first]] = dep_all[g]
            m_set[at[first]] = True
            T[at] = test_T
        out[ys, xs] = F
        alpha_map[ys, xs] = _F(1.0) - T
        depth_map[ys, xs] = D
        median_map[ys, xs] = M
        t_map[ys, xs] = T
    return dict(features=out, alpha=alpha_map, depth=depth_map, median=median_map, T=t_map)
