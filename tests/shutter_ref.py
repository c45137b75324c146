"""NumPy statement of a shutter frame's layers (include/bhr.h: bhr_render_shutter): the sequential f32 sum of the samples'
layers, then one product with the f32 reciprocal of their number."""
import numpy as np


def resolve(layers) -> np.ndarray:
    """layers: the n samples' (H, W, 3) float32 layers, in order.  acc = L_0; acc = acc + L_j, one f32 addition per channel;
    the frame's layer is acc * (f32(1) / f32(n)) -- the reciprocal rounded once, the product once.  n = 1: L_0 itself."""
    layers = [np.asarray(l) for l in layers]
    n = len(layers)
    if n < 1:
        raise ValueError("a shutter frame has at least one sample")
    for l in layers:
        if l.dtype != np.float32 or l.shape != layers[0].shape:
            raise ValueError("the samples' layers are float32 arrays of one shape")
    if n == 1:
        return layers[0].copy()
    acc = layers[0].copy()
    for l in layers[1:]:
        acc = acc + l                       # float32 + float32: one rounding
    inv = np.float32(1) / np.float32(n)
    return acc * inv
