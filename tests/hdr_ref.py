"""NumPy restatement of the HDR video stream's conversion (include/bhr_output.h: bhr_y4m_open_hdr; csrc/hdr_stream.hip).

``encode(h, transfer, exposure, white_nits)`` is the truth: the formulas in binary64 on the f32 plane the device holds.
``encode(..., dtype=np.float32)`` follows the kernel operation by operation -- every product, sum and quotient rounded to f32 once,
in the kernel's order -- with NumPy's f32 exp2, log2, logarithm and square root in place of the device library's.  Both return the
frame's code planes and its light levels.
"""
import numpy as np

TRANSFERS = ("pq", "hlg")

M_709_TO_2020 = ((0.6274, 0.3293, 0.0433), (0.0691, 0.9195, 0.0114), (0.0164, 0.0880, 0.8956))     # BT.2087
PQ_M1, PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
PQ_C1, PQ_C2, PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
HLG_A, HLG_B, HLG_C = 0.17883277, 0.28466892, 0.55991073
HLG_SCENE_WHITE = 0.265                      # scene value 1.0 -> the 75 % reference white (BT.2408)
LUMA = (0.2627, 0.6780, 0.0593)              # BT.2020 non-constant luminance
CB_DIV, CR_DIV = 1.8814, 1.4746


def _pow(x, e, dtype):
    """x^e: the power function in binary64; in f32 the kernel's exp2f(e * log2f(x)), the product rounded once."""
    if dtype is np.float64:
        return np.power(x, e)
    with np.errstate(divide="ignore"):
        return np.exp2(e * np.log2(x)).astype(dtype)


def pq_oetf(y, dtype=np.float64):
    """ST 2084: display luminance / 10000 nits, in [0, 1] -> E'."""
    T = dtype
    y = np.asarray(y, dtype=T)
    p = _pow(y, T(PQ_M1), T)
    return _pow((T(PQ_C1) + T(PQ_C2) * p) / (T(1.0) + T(PQ_C3) * p), T(PQ_M2), T)


def hlg_oetf(e, dtype=np.float64):
    """BT.2100 HLG: scene light E in [0, 1] -> E'."""
    T = dtype
    e = np.asarray(e, dtype=T)
    low = e <= T(1.0) / T(12.0)
    arg = T(12.0) * e - T(HLG_B)
    hi = T(HLG_A) * np.log(np.where(low, T(1.0), arg)) + T(HLG_C)
    return np.where(low, np.sqrt(T(3.0) * e), hi).astype(T)


def gain_of(exposure, dtype=np.float64):
    """(float)exp2((double)exposure_stops) of an f32 exposure."""
    return dtype(np.float32(2.0 ** float(np.float32(exposure))))


def linear_2020(h, exposure, dtype=np.float64):
    """v = h * gain, then (R, G, B) = M . v with each row summed as (m0 r + m1 g) + m2 b: (H, W, 3)."""
    T = dtype
    v = np.asarray(h, dtype=np.float32).astype(T) * gain_of(exposure, T)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([(T(m[0]) * r + T(m[1]) * g) + T(m[2]) * b for m in M_709_TO_2020], axis=-1)


def transfer_of(lin, transfer, white_nits, dtype=np.float64):
    """The non-linear R'G'B' of linear BT.2020 values."""
    T = dtype
    if transfer == "pq":
        scale = T(np.float32(white_nits)) / T(10000.0)
        return pq_oetf(np.minimum(lin * scale, T(1.0)), T)
    if transfer == "hlg":
        return hlg_oetf(np.minimum(lin * T(HLG_SCENE_WHITE), T(1.0)), T)
    raise ValueError(f"transfer must be one of {TRANSFERS}, got {transfer!r}")


def luma(e, dtype=np.float64):
    T = dtype
    return (T(LUMA[0]) * e[..., 0] + T(LUMA[1]) * e[..., 1]) + T(LUMA[2]) * e[..., 2]


def code_y(y, dtype=np.float64):
    T = dtype
    return np.clip(np.floor(T(876.0) * y + T(64.5)), 64, 940).astype(np.uint16)


def code_c(c, dtype=np.float64):
    T = dtype
    return np.clip(np.floor(T(896.0) * c + T(512.5)), 64, 960).astype(np.uint16)


def encode(h, transfer, exposure=0.0, white_nits=203.0, dtype=np.float64):
    """(H, W, 3) f32 scene-linear BT.709 plane, H and W even -> dict(y (H, W), cb, cr (H/2, W/2) uint16 codes, max_nits, mean_nits:
    the frame's largest and mean min(white_nits * max(R, G, B), 10000); both 0 for HLG)."""
    T = dtype
    h = np.asarray(h, dtype=np.float32)
    if h.ndim != 3 or h.shape[2] != 3 or h.shape[0] % 2 or h.shape[1] % 2:
        raise ValueError(f"expected an (H, W, 3) plane with even H and W, got {h.shape}")
    lin = linear_2020(h, exposure, T)
    e = transfer_of(lin, transfer, white_nits, T)
    a, b, c, d = e[0::2, 0::2], e[0::2, 1::2], e[1::2, 0::2], e[1::2, 1::2]
    m = ((a + b) + (c + d)) * T(0.25)
    ym = luma(m, T)
    out = dict(y=code_y(luma(e, T), T), cb=code_c((m[..., 2] - ym) / T(CB_DIV), T), cr=code_c((m[..., 0] - ym) / T(CR_DIV), T),
               max_nits=0.0, mean_nits=0.0)
    if transfer == "pq":
        nits = np.minimum(T(np.float32(white_nits)) * lin.max(axis=-1), T(10000.0))
        out["max_nits"] = float(nits.max())
        out["mean_nits"] = float(nits.astype(np.float64).mean())          # the device sums in binary64 too
    return out


def light_levels(frames_levels):
    """(MaxCLL, MaxFALL) of a stream from its frames' (max_nits, mean_nits) pairs."""
    frames_levels = list(frames_levels)
    if not frames_levels:
        return 0.0, 0.0
    return max(f[0] for f in frames_levels), max(f[1] for f in frames_levels)


class Tally:
    """The issue's criterion for a stream against the restatement: every sample within one code, and at most 1 % of the samples
    of each plane -- Y, Cb, Cr -- different at all.  A frame's plane of a hundred samples or more is held to the cap by itself.
    Below that, 1 % is less than one sample and the cap would say "none", which correctly rounded f32 arithmetic does not promise
    (a sample lies within f32 rounding of a code boundary with probability ~1e-3): there the cap holds over the plane's samples
    of all frames added under one key (the tests use the transfer, at one frame size), as the issue states its own trial's
    shares -- per transfer and plane."""

    def __init__(self):
        self.off, self.n = {}, {}

    def add(self, key, got, want, tag=""):
        for name, g in zip(("y", "cb", "cr"), got):
            w = want[name]
            assert g.shape == w.shape and g.dtype == np.uint16, f"{tag} {name}: {g.dtype} {g.shape}, expected uint16 {w.shape}"
            diff = np.abs(g.astype(np.int32) - w.astype(np.int32))
            assert diff.max() <= 1, f"{tag} {name}: {int(diff.max())} codes from the restatement at {np.unravel_index(diff.argmax(), diff.shape)}"
            off = int((diff != 0).sum())
            if diff.size >= 100:
                assert off <= 0.01 * diff.size, f"{tag} {name}: {off} of {diff.size} samples are one code off (cap: 1 %)"
            self.off[key, name] = self.off.get((key, name), 0) + off
            self.n[key, name] = self.n.get((key, name), 0) + diff.size

    def check(self):
        """Asserts the pooled cap; returns the shares as text."""
        parts = []
        for k in sorted(self.n):
            assert self.off[k] <= 0.01 * self.n[k], f"{k[0]} {k[1]}: {self.off[k]} of {self.n[k]} samples are one code off (cap: 1 %)"
            parts.append(f"{k[0]} {k[1]} {self.off[k]}/{self.n[k]}")
        return ", ".join(parts)
