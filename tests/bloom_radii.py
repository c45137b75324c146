"""The radius classes of the split-f16 post-pass (csrc/bloom.hip): R = int(0.02 W) (render.py:3914, context.hip), weight
table count NT = (R + 15) // 16 + 1 (bhr_split_nt), split kernels up to NT = 12, i.e. W <= 8849 (split_ok).  The frame
shapes tests/test_gpu_bloom_radii.py runs and the synthetic layers it blurs."""
import numpy as np

SPLIT_NT_MAX = 12
SPLIT_W_MAX = 8849


def radius(width: int) -> int:
    return int(width * 0.02)            # (int32_t)(width * 0.02) in binary64, as the library computes it


def split_nt(width: int) -> int:
    return (radius(width) + 15) // 16 + 1


# both ends of every table count's width range
NT_ENDS = {1: (1, 49), 2: (50, 849), 3: (850, 1649), 4: (1650, 2449), 5: (2450, 3249), 6: (3250, 4049),
           7: (4050, 4849), 8: (4850, 5649), 9: (5650, 6449), 10: (6450, 7249), 11: (7250, 8049), 12: (8050, 8849)}
# QHD and 5K, and the width classes the ends miss (every end has W % 4 in {1, 2}): W % 4 == 0 with W % 32 != 0 (the
# cooperative V epilogue next to a partial right strip) and W % 32 == 0
EXTRA_WIDTHS = (32, 40, 844, 1648, 2560, 3252, 5120, 6464, 8832, 8844)
WIDTHS = tuple(sorted({w for ends in NT_ENDS.values() for w in ends} | set(EXTRA_WIDTHS)))

SMALL_HEIGHTS = (1, 7, 31, 33)
TALL_HEIGHTS = tuple(32 * k + 5 for k in range(1, 10))          # 37 ... 293


def shapes():
    """(W, H) pairs: every width twice, once with a height below 34 and once with a 32 k + 5 one; at NT >= 8 the second
    is below the radius (the V pass's band is wider than the image)"""
    out = []
    for i, w in enumerate(WIDTHS):
        tall = TALL_HEIGHTS[i % len(TALL_HEIGHTS)]
        if split_nt(w) >= 8:
            below = [h for h in TALL_HEIGHTS if h < radius(w)]
            tall = below[i % len(below)]
        out += [(w, SMALL_HEIGHTS[i % len(SMALL_HEIGHTS)]), (w, tall)]
    return out


def synthetic_layers(W: int, H: int, seed: int):
    """(disk, bg), (H, W, 3) f32: a faint floor (1e-6 .. 1e-4), sparse random points, a bright block and bright first and
    last rows and columns (the edge renormalisation); disk values in [0, 1] as a march writes them.  bg is random in
    [0, 0.7): the combine clips some pixels."""
    rng = np.random.default_rng(seed)
    disk = (rng.random((H, W, 3), dtype=np.float32) * np.float32(9.9e-5) + np.float32(1e-6)).astype(np.float32)
    n = max(1, W * H // 40)
    ys, xs = rng.integers(0, H, n), rng.integers(0, W, n)
    disk[ys, xs] = rng.random((n, 3), dtype=np.float32)
    disk[H // 3:H // 3 + max(1, H // 4), W // 5:W // 5 + max(1, W // 3)] = np.array([0.6, 0.9, 0.3], np.float32)
    disk[0, :] = 0.9
    disk[-1, :] = np.array([0.2, 0.7, 1.0], np.float32)
    disk[:, 0] = 0.8
    disk[:, -1] = 1.0
    bg = (rng.random((H, W, 3), dtype=np.float32) * np.float32(0.7)).astype(np.float32)
    return disk, bg
