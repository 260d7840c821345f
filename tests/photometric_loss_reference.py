"""gs_photometric_loss (include/gs3d_hip.h) restated in numpy: the yardstick of tests/test_gpu_photometric_loss.py, itself held to
torch.autograd and to binary80 by tests/test_photometric_loss_api.py.

THE FUNCTION (exact real arithmetic).  x = image, y = target, [H][W][3]; g[k] = exp(-(k - 5)^2 / 4.5) / sum, k = 0..10; w = g g^T;
a* = the 11 x 11 correlation of a map with w per channel, zeros outside the image; n = 3 H W; C1 = 1e-4, C2 = 9e-4.
    mu1 = x*   mu2 = y*   s11 = (x^2)* - mu1^2   s22 = (y^2)* - mu2^2   s12 = (x y)* - mu1 mu2
    A = 2 mu1 mu2 + C1    B = 2 s12 + C2    C = mu1^2 + mu2^2 + C1    D = s11 + s22 + C2    S = A B / (C D)
    l1 = sum |x - y| / n    ssim = sum S / n    mse = sum (x - y)^2 / n    loss = (1 - lam) l1 + lam (1 - ssim)
    P1 = 2 mu2 (B - A) / (C D) + 2 mu1 S (1 / D - 1 / C)      P2 = -S / D      P3 = 2 A / (C D)
    d loss / d x = (1 - lam) sign(x - y) / n - (lam / n) (P1* + 2 x P2* + y P3*)        sign(0) = 0
lam == 0: the window is not evaluated; ssim is NaN ("not evaluated"), loss = l1, the gradient is sign(x - y) / n.

evaluate() is this text in the dtype asked for (binary64 by default; np.longdouble is the "exact" value the API test compares
with), the correlation separable (rows, then columns), which the contract permits.

THE BOUND.  The contract leaves the association open, so bound() follows the LOOSEST permitted one and counts, to first order in
u = 2^-53, the roundings on the way to every value; E(q) below is the bound on |computed q - exact q| in units of u.  A rounding
of a sum or difference is charged to the sum of its constituents' absolute values, never to the (possibly cancelled) result.
  * A correlation a*: direct, 121 terms, no fused operation: each term carries the roundings of g_i and g_j (1 + 1: g is the
    binary64 rounding of its definition), of their product w_ij (1) and of w_ij a (1), and the 121 terms are added in any order
    (120 roundings, each on a partial sum of at most |a|*).   K_CONV = 4 + 120 = 124:   E(a*) = K_CONV |a|*.
    (x^2 and x y are exact in binary64: products of two binary32 values.)   The separable form counts 2 (1 + 1 + 10) = 24.
  * The cancelling intermediates, with M11 = (x^2)* + mu1^2, M12 = |x y|* + |mu1 mu2|:
        E(s11) = K_CONV (x^2)* + 2 |mu1| E(mu1) + mu1^2 [the square] + M11 [the subtraction];      E(s22) alike;
        E(s12) = K_CONV |x y|* + |mu1| E(mu2) + |mu2| E(mu1) + |mu1 mu2| + M12.
  * E(A) = 2 (|mu1| E(mu2) + |mu2| E(mu1)) + 2 |mu1 mu2| [product] + (2 |mu1 mu2| + C1) [sum] + C1 [the constant's rounding]
    E(B) = 2 E(s12) + (2 M12 + C2) + C2
    E(C) = 2 |mu1| E(mu1) + 2 |mu2| E(mu2) + (mu1^2 + mu2^2) [squares] + 2 (mu1^2 + mu2^2 + C1) [two sums] + C1
    E(D) = E(s11) + E(s22) + 2 (M11 + M22 + C2) + C2
  * The divisions, each by its condition: C >= C1 > 0 and D >= C2 > 0 in exact arithmetic; rC = E(C) / C, rD = E(D) / D are the
    relative errors 1 / C and 1 / D inherit.  The loosest form takes the two reciprocals, multiplies them and multiplies on:
        E(S)  = (|B| E(A) + |A| E(B)) / (C D) + |S| (rC + rD + K_S),    K_S = 6  (1/C, 1/D, their product, A B, the product; +1)
        E(P3) = 2 E(A) / (C D) + |P3| (rC + rD + 5)
        E(P2) = E(S) / D + |P2| (rD + 3)
        E(B - A) = E(A) + E(B) + (|A| + |B|)
        T1 = 2 mu2 (B - A) / (C D):  E(T1) = 2 (E(mu2) |B - A| + |mu2| E(B - A)) / (C D) + |T1| (rC + rD + 6)
        V = 1 / D - 1 / C:           E(V)  = (rD + 1) / D + (rC + 1) / C + (1 / D + 1 / C)
        T2 = 2 mu1 S V:              E(T2) = 2 (E(mu1) |S V| + |mu1| E(S) |V| + |mu1 S| E(V)) + 4 |T2|
        E(P1) = E(T1) + E(T2) + (|T1| + |T2|)
  * The second correlation: E(P*) = E(P)* + K_CONV |P|*  (the P maps are kept in binary64: no rounding between the passes).
  * G = P1* + 2 x P2* + y P3*, MG = |P1|* + 2 |x| |P2|* + |y| |P3|*:   E(G) = E(P1*) + 2 |x| E(P2*) + |y| E(P3*) + 4 MG
    (two products, two sums).  c1 = (1 - lam) / n (2 roundings), c2 = lam / n (1), the product c2 G (1), the difference (1):
        E(grad) = c2 E(G) + 2 c2 MG + 2 c1 + (c1 + c2 MG).
  * A grad_rgb element is that value rounded once to binary32:
        |got - want| <= u E(grad) (1 + SECOND_ORDER) + 2^-24 (|want| + u E(grad)) + 2^-149.
    SECOND_ORDER = 2^-20 covers the products of two errors the first-order count drops (each at most u rD ~ 1e-8 of a term
    on the listed images).
  * The terms, n addends summed in any order and divided by n:  l1: each |x - y| one rounding: (n + 2) u l1.   mse: the
    difference, the square: (n + 4) u mse.   ssim: u (sum E(S) + (n + 1) sum |S|) / n.   loss: (1 - lam) E(l1) + lam E(ssim)
    + 3 u ((1 - lam) l1 + lam (1 + |ssim|))  (1 - lam, the two products, 1 - ssim, the sum: at most three on either addend).
None of these constants was fitted to a device's output.

mutate= takes ONE of MUTATIONS: single-term slips of the text above, each of which the API test shows to miss the bound by 10 x.
"""
import numpy as np

C1, C2 = 1e-4, 9e-4
U = 2.0 ** -53
RADIUS = 5
K_CONV = 124
K_S = 6
SECOND_ORDER = 2.0 ** -20
TERMS = ("loss", "l1", "ssim", "mse")
MUTATIONS = ("drop_P2", "drop_P3", "replicate_padding", "window_not_normalised", "sign0_is_1", "swap_C1_C2", "mean_over_HW", "sigma_1")


def window(dtype=np.float64, sigma=1.5, normalise=True):
    """g[0..10].  binary64: the binary64 rounding of the definition (formed in binary80, rounded once); longdouble: unrounded."""
    k = np.arange(11, dtype=np.longdouble)
    g = np.exp(-((k - 5) ** 2) / (2 * np.longdouble(sigma) ** 2))
    if normalise:
        g = g / g.sum()
    return g.astype(dtype)


def correlate(a, g, replicate=False):
    """a* for a [H][W][3] map: rows, then columns; zeros (or, the mutation, the edge value) outside the image."""
    h, w = a.shape[:2]
    p = np.pad(a, ((0, 0), (RADIUS, RADIUS), (0, 0)), mode="edge" if replicate else "constant")
    rows = np.zeros_like(a)
    for k in range(11):
        rows = rows + g[k] * p[:, k:k + w]
    p = np.pad(rows, ((RADIUS, RADIUS), (0, 0), (0, 0)), mode="edge" if replicate else "constant")
    out = np.zeros_like(a)
    for k in range(11):
        out = out + g[k] * p[k:k + h]
    return out


def _rgb(a, dtype):
    a = np.asarray(a)
    assert a.ndim == 3 and a.shape[2] in (3, 4) and a.dtype == np.float32, (a.shape, a.dtype)
    return a[..., :3].astype(dtype)


def evaluate(x, y, lam, dtype=np.float64, mutate=None, parts=False):
    """dict(terms = [loss, l1, ssim, mse], grad = d loss / d x, [H][W][3]) in `dtype`; parts=True adds the intermediates."""
    assert mutate is None or mutate in MUTATIONS, mutate
    x, y = _rgb(x, dtype), _rgb(y, dtype)
    assert x.shape == y.shape
    h, w = x.shape[:2]
    one, two = dtype(1), dtype(2)
    lam = dtype(lam)
    n = dtype(h * w if mutate == "mean_over_HW" else 3 * h * w)
    with np.errstate(all="ignore"):
        d = x - y
        sign = np.sign(d)
        if mutate == "sign0_is_1":
            sign = np.where(d == 0, one, sign)
        l1, mse = np.abs(d).sum() / n, (d * d).sum() / n
        if lam == 0:
            out = dict(terms=np.array([l1, l1, dtype(np.nan), mse], dtype), grad=(one - lam) * sign / n)
            if parts:
                out.update(x=x, y=y, n=n)
            return out
        c1, c2 = dtype(1) / dtype(10000), dtype(9) / dtype(10000)
        if dtype == np.float64:
            c1, c2 = np.float64(C1), np.float64(C2)
        if mutate == "swap_C1_C2":
            c1, c2 = c2, c1
        g = window(dtype, sigma=1.0 if mutate == "sigma_1" else 1.5, normalise=mutate != "window_not_normalised")

        def conv(a):
            return correlate(a, g, replicate=mutate == "replicate_padding")
        m1, m2 = conv(x), conv(y)
        s11, s22, s12 = conv(x * x) - m1 * m1, conv(y * y) - m2 * m2, conv(x * y) - m1 * m2
        A, B, C, D = two * m1 * m2 + c1, two * s12 + c2, m1 * m1 + m2 * m2 + c1, s11 + s22 + c2
        S = A * B / (C * D)
        ssim = S.sum() / n
        P1 = two * m2 * (B - A) / (C * D) + two * m1 * S * (one / D - one / C)
        P2, P3 = -S / D, two * A / (C * D)
        G = conv(P1)
        if mutate != "drop_P2":
            G = G + two * x * conv(P2)
        if mutate != "drop_P3":
            G = G + y * conv(P3)
        grad = (one - lam) * sign / n - (lam / n) * G
        loss = (one - lam) * l1 + lam * (one - ssim)
    out = dict(terms=np.array([loss, l1, ssim, mse], dtype), grad=grad)
    if parts:
        out.update(x=x, y=y, m1=m1, m2=m2, A=A, B=B, C=C, D=D, S=S, P1=P1, P2=P2, P3=P3, n=n)
    return out


def bound(x, y, lam):
    """dict(grad = [H][W][3], grad64 = the same without the rounding to binary32 (a binary64 evaluation's bound), terms = [4]): the
    contract's bound on |got - exact| of gs_photometric_loss (docstring above), from the binary64 intermediates.  An element the arithmetic takes a NaN or an infinity to has a NaN or infinite bound."""
    lam = float(lam)
    q = evaluate(x, y, 1.0 if lam == 0 else lam, parts=True)
    x, y, n = q["x"], q["y"], float(q["n"])
    with np.errstate(all="ignore"):
        d = x - y
        l1, mse = np.abs(d).sum() / n, (d * d).sum() / n
        e_l1, e_mse = (n + 2) * l1, (n + 4) * mse
        if lam == 0:
            want = np.sign(d) / n
            e_grad = np.full(x.shape, 3.0 / n)                        # 1 - lam, the division, the product with the sign
            grad = U * e_grad * (1 + SECOND_ORDER) + 2.0 ** -24 * (np.abs(want) + U * e_grad) + 2.0 ** -149
            return dict(grad=grad, grad64=U * e_grad * (1 + SECOND_ORDER), terms=U * np.array([e_l1 + 3 * l1, e_l1, np.nan, e_mse]))
        g = window()

        def conv(a):
            return correlate(a, g)
        m1, m2, A, B, C, D, S = (q[k] for k in ("m1", "m2", "A", "B", "C", "D", "S"))
        am1, am2, am12 = np.abs(m1), np.abs(m2), np.abs(m1 * m2)
        q11, q22, q12 = conv(x * x), conv(y * y), conv(np.abs(x * y))
        e_m1, e_m2 = K_CONV * conv(np.abs(x)), K_CONV * conv(np.abs(y))
        M11, M22, M12 = q11 + m1 * m1, q22 + m2 * m2, q12 + am12
        e_s11 = K_CONV * q11 + 2 * am1 * e_m1 + m1 * m1 + M11
        e_s22 = K_CONV * q22 + 2 * am2 * e_m2 + m2 * m2 + M22
        e_s12 = K_CONV * q12 + am1 * e_m2 + am2 * e_m1 + am12 + M12
        e_A = 2 * (am1 * e_m2 + am2 * e_m1) + 2 * am12 + (2 * am12 + C1) + C1
        e_B = 2 * e_s12 + (2 * M12 + C2) + C2
        e_C = 2 * am1 * e_m1 + 2 * am2 * e_m2 + (m1 * m1 + m2 * m2) + 2 * (m1 * m1 + m2 * m2 + C1) + C1
        e_D = e_s11 + e_s22 + 2 * (M11 + M22 + C2) + C2
        ok = (C > 0) & (D > 0) & (U * e_D < D / 4) & (U * e_C < C / 4)   # (elsewhere a division is not conditioned at all)
        rC, rD = np.where(ok, e_C / C, np.inf), np.where(ok, e_D / D, np.inf)
        iCD = 1 / (C * D)
        aS, aP2, aP3 = np.abs(S), np.abs(q["P2"]), np.abs(q["P3"])
        e_S = (np.abs(B) * e_A + np.abs(A) * e_B) * iCD + aS * (rC + rD + K_S)
        e_P3 = 2 * e_A * iCD + aP3 * (rC + rD + 5)
        e_P2 = e_S / D + aP2 * (rD + 3)
        e_BA = e_A + e_B + (np.abs(A) + np.abs(B))
        T1 = 2 * m2 * (B - A) * iCD
        V = 1 / D - 1 / C
        T2 = 2 * m1 * S * V
        e_T1 = 2 * (e_m2 * np.abs(B - A) + am2 * e_BA) * iCD + np.abs(T1) * (rC + rD + 6)
        e_V = (rD + 1) / D + (rC + 1) / C + (1 / D + 1 / C)
        e_T2 = 2 * (e_m1 * aS * np.abs(V) + am1 * e_S * np.abs(V) + am1 * aS * e_V) + 4 * np.abs(T2)
        e_P1 = e_T1 + e_T2 + (np.abs(T1) + np.abs(T2))
        aP1 = np.abs(T1) + np.abs(T2)
        cP1, cP2, cP3 = conv(aP1), conv(aP2), conv(aP3)
        e_cP1, e_cP2, e_cP3 = conv(e_P1) + K_CONV * cP1, conv(e_P2) + K_CONV * cP2, conv(e_P3) + K_CONV * cP3
        ax, ay = np.abs(x), np.abs(y)
        MG = cP1 + 2 * ax * cP2 + ay * cP3
        e_G = e_cP1 + 2 * ax * e_cP2 + ay * e_cP3 + 4 * MG
        c1, c2 = (1 - lam) / n, lam / n
        e_grad = c2 * e_G + 2 * c2 * MG + 2 * c1 + (c1 + c2 * MG)
        want = q["grad"]
        grad = U * e_grad * (1 + SECOND_ORDER) + 2.0 ** -24 * (np.abs(want) + U * e_grad) + 2.0 ** -149
        ssim = S.sum() / n
        e_ssim = (e_S.sum() + (n + 1) * aS.sum()) / n
        e_loss = (1 - lam) * e_l1 + lam * e_ssim + 3 * ((1 - lam) * l1 + lam * (1 + abs(ssim)))
        terms = U * (1 + SECOND_ORDER) * np.array([e_loss, e_l1, e_ssim, e_mse])
    return dict(grad=grad, grad64=U * e_grad * (1 + SECOND_ORDER), terms=terms)
