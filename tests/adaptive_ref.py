"""The criterion of adaptive supersampling (bhr_set_adaptive_supersample, include/bhr.h steps 2-3) in NumPy: the statement
the GPU tests hold the detect kernel to, bit for bit."""
import numpy as np


def contrast(bg, disk):
    """(H, W, 3) f32 layers of the k = 1 frame -> (H, W) f32: c(p) = the largest |L[p] - L[n]| over the edge neighbours n
    of p inside the frame, both layers and the three channels; each difference one f32 subtraction.  A 1 x 1 frame has 0."""
    bg, disk = np.asarray(bg, dtype=np.float32), np.asarray(disk, dtype=np.float32)
    assert bg.shape == disk.shape and bg.ndim == 3
    c = np.zeros(bg.shape[:2], dtype=np.float32)
    for layer in (bg, disk):
        dx = np.abs(layer[:, 1:] - layer[:, :-1]).astype(np.float32).max(axis=2)     # between columns i and i + 1
        dy = np.abs(layer[1:, :] - layer[:-1, :]).astype(np.float32).max(axis=2)     # between rows j and j + 1
        c[:, 1:] = np.maximum(c[:, 1:], dx)
        c[:, :-1] = np.maximum(c[:, :-1], dx)
        c[1:, :] = np.maximum(c[1:, :], dy)
        c[:-1, :] = np.maximum(c[:-1, :], dy)
    return c


def refined_mask(bg, disk, threshold):
    """(H, W) bool: the pixels that get the k x k rays, c(p) > T as an f32 comparison (T = +inf: none, T < 0: all)."""
    t = np.float32(threshold)
    assert t == t, "NaN threshold"
    return contrast(bg, disk) > t
