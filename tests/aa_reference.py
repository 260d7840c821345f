"""The antialiased mode's opacity factor (gs_set_antialiased) in float64, from np_reference.preprocess's 2D covariance, and the
bound within which the binary32 kernel's factor must agree with it.

    comp = sqrt(max(0, det(cov2D) / det(cov2D + 0.3 I)))        opacity' = opacity * comp

The pipeline evaluates it in binary32 from the same products that give the dilated matrix; np_reference returns that dilated
matrix (cov2d = [a + 0.3, b, c + 0.3]) and its determinant."""
import numpy as np

import float64_check as f64
import np_reference as npr

EPS = 2.0 ** -24


def comp64(pre, rules=None, sqrt=True, raw_from_dilated=False):
    """float64 comp of every Gaussian of `pre` (np_reference.preprocess).  sqrt / raw_from_dilated: mutations the tests use to
    show that the check below notices a missing square root or det(cov2D) taken from the dilated matrix."""
    R = npr.rules_with(rules)
    a, b, c = pre["cov2d"].T
    det = pre["det"]
    if raw_from_dilated:
        det_raw = det
    else:
        a0, c0 = a - R["dilation"], c - R["dilation"]
        det_raw = a0 * c0 - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.fmax(0.0, det_raw / det)
    return np.fmin(1.0, np.sqrt(ratio) if sqrt else ratio)


def comp_tolerance(pre):
    """First-order bound on |comp_gpu^2 - comp64^2|, per Gaussian, with the error model of float64_check.py:

      * every entry of the binary32 2D covariance is within delta = K_COV ulp of its terms' magnitude of the exact value
        (delta = K_COV EPS max(cov_scale, lambda_max): the model float64_check.py already holds the conic to);
      * det_raw = a0 c0 - b b cancels: its error is delta (|a0| + |c0| + 2|b|) + delta^2 from the entries, plus one rounding
        of each product and of the difference, 2 EPS (|a0 c0| + b^2);  det of the dilated matrix likewise, plus the rounding of
        each + 0.3 (EPS (|a| + |c|) through the other factor);
      * comp^2 = det_raw / det:  |d comp^2| <= (|d det_raw| + comp^2 |d det|) / det;
      * the rounding of the quotient, of the square root and of opacity * comp, and reading comp back as opacity' / opacity:
        1 + 2 + 2 = 5 EPS relative on comp^2 (k = 5; the square doubles a relative error).
    Everything is multiplied by float64_check.SLACK (2), the suite's margin on a modelled uncertainty."""
    a, b, c = pre["cov2d"].T
    det = pre["det"]
    dil = 0.3
    a0, c0 = a - dil, c - dil
    half = np.sqrt((0.5 * (a - c)) ** 2 + b * b)
    lmax = pre["mid"] + half
    delta = f64.K_COV * EPS * np.maximum(pre["cov_scale"], lmax)
    d_raw = delta * (np.abs(a0) + np.abs(c0) + 2 * np.abs(b)) + delta ** 2 + 2 * EPS * (np.abs(a0 * c0) + b * b)
    d_dil = delta * (np.abs(a) + np.abs(c) + 2 * np.abs(b)) + delta ** 2 + 2 * EPS * (np.abs(a * c) + b * b) + EPS * (np.abs(a) + np.abs(c))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.clip((a0 * c0 - b * b) / det, 0.0, 1.0)
        first = (d_raw + ratio * d_dil) / det
    return f64.SLACK * (first + 5 * EPS * ratio)


def comp_violations(comp_gpu, pre, want):
    """Mask of the Gaussians whose binary32 comp (opacity' / opacity) is outside the bound around `want` (a float64 comp)."""
    g = np.asarray(comp_gpu, np.float64)
    return ~(np.abs(g * g - want * want) <= comp_tolerance(pre))
