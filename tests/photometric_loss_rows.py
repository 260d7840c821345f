"""A model of how gs_loss.hip PARTITIONS its three sums -- sum |x - y|, sum S, sum (x - y)^2 -- into the rows of partial sums that
k_loss_finish adds: which elements meet in which row, not how a workgroup adds them.  Built from the per-element values of
tests/photometric_loss_reference.py, so tests/test_photometric_loss_api.py can show, without a GPU, that one missing, doubled or
stale row at any size of photometric_loss_images.REDUCTION_SIZES breaks the bound the GPU tests hold the device to.
  lambda > 0   k_loss_ssim: one row per TILE x TILE tile, all three channels, at  blockIdx.y * gridDim.x + blockIdx.x.
  lambda = 0   k_loss_l1: element e = 3 pixel + channel belongs to workgroup (e / THREADS) mod rows, rows = min(ceil(E / THREADS),
               L1_GROUPS): the grid stride under the cap.  The S column is zero (k_loss_finish does not read it into a term)."""
import numpy as np

import photometric_loss_images as pli
import photometric_loss_reference as plr


def partial_rows(x, y, lam, q=None):
    """[rows][3] in binary64: the sums of |d|, S, d^2 over each row's elements.  q: evaluate(x, y, lam, parts=True), if at hand."""
    q = plr.evaluate(x, y, lam, parts=True) if q is None else q
    d = q["x"] - q["y"]
    h, w = d.shape[:2]
    per = np.stack([np.abs(d), q["S"] if lam != 0 else np.zeros_like(d), d * d])          # [3][h][w][3]
    if lam != 0:
        gy, gx = pli.ssim_rows(h, w)
        padded = np.zeros((3, gy * pli.TILE, gx * pli.TILE, 3))
        padded[:, :h, :w] = per
        return padded.reshape(3, gy, pli.TILE, gx, pli.TILE, 3).sum(axis=(2, 4, 5)).reshape(3, gy * gx).T.copy()
    rows, e = pli.l1_rows(h, w), 3 * h * w
    passes = -(-e // (rows * pli.THREADS))
    padded = np.zeros((3, passes * rows * pli.THREADS))
    padded[:, :e] = per.reshape(3, e)
    return padded.reshape(3, passes, rows, pli.THREADS).sum(axis=(1, 3)).T.copy()
