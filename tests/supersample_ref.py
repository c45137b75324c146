"""The box filter of supersampling (bhr_set_supersample, include/bhr.h) in NumPy: the statement the GPU tests hold the
march's in-wave resolve to, bit for bit."""
import numpy as np


def _pairwise(x, axis):
    """Pairwise f32 tree along `axis` (a power-of-two length): adjacent pairs, then pairs of those sums, and so on."""
    x = np.asarray(x, dtype=np.float32)
    while x.shape[axis] > 1:
        n = x.shape[axis]
        x = (np.take(x, np.arange(0, n, 2), axis=axis) + np.take(x, np.arange(1, n, 2), axis=axis)).astype(np.float32)
    return np.squeeze(x, axis=axis)


def box_resolve(fine, k):
    """(k H, k W, 3) f32 -> (H, W, 3): each sub-sample row summed as a pairwise tree, the k row sums by the same tree, one
    product with 1 / k^2 (exact: k is a power of two)."""
    fine = np.asarray(fine, dtype=np.float32)
    h, w = fine.shape[0] // k, fine.shape[1] // k
    x = fine.reshape(h, k, w, k, fine.shape[2])
    rows = _pairwise(x, axis=3)                  # (h, k, w, c): the sub-sample rows
    return (_pairwise(rows, axis=1) * np.float32(1.0 / (k * k))).astype(np.float32)
