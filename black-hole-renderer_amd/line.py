"""The Kerr line profile on the host (include/bhr.h "Kerr line profile"): the settings and their checks, the conversion of a
device row's integers into flux, the profile's moments and edges, the redshift map's colours and the .npz writer.

The device adds, per counted disk crossing, the integer Q = llrint(w * unit) to the cell of g's bin, w = g^p eps dOmega T and
unit = 2^32 / 1.5^p.  Nothing here needs the device or the library."""
from __future__ import annotations

from typing import Optional

import numpy as np

G_CAP = 1.5                 # the g-factor's cap (BHR_G_FACTOR_CAP)
MAX_BINS = 4096             # BHR_LINE_MAX_BINS
EMISSIVITIES = ("powerlaw", "texture")
ORDERS = ("first", "all")
DEFAULTS = dict(n_bins=256, g_range=(0.0, 2.0), index=3.0, power=4.0, emissivity="powerlaw", orders="first", r_inner=None, r_outer=None)
DEFAULT_ENERGY_KEV = 6.4    # Fe K alpha


def check_settings(n_bins=256, g_range=(0.0, 2.0), index=3.0, power=4.0, emissivity="powerlaw", orders="first",
                   r_inner: Optional[float] = None, r_outer: Optional[float] = None) -> dict:
    """The settings of a line as a dict, checked as bhr_set_kerr_line checks them (the annulus against the disk's is the
    library's to check); ValueError naming the field."""
    if int(n_bins) != n_bins or not 1 <= int(n_bins) <= MAX_BINS:
        raise ValueError(f"line profile: n_bins {n_bins!r} (1 .. {MAX_BINS})")
    try:
        g_min, g_max = (float(v) for v in g_range)
    except (TypeError, ValueError):
        raise ValueError(f"line profile: range {g_range!r} (two numbers, g_min < g_max)") from None
    if not (np.isfinite(g_min) and np.isfinite(g_max) and g_min < g_max):
        raise ValueError(f"line profile: range ({g_min}, {g_max}): finite, g_min < g_max")
    if not 0.0 <= float(index) <= 16.0:
        raise ValueError(f"line profile: emissivity index {index!r} (0 .. 16)")
    if not 0.0 <= float(power) <= 8.0:
        raise ValueError(f"line profile: power {power!r} (0 .. 8)")
    if emissivity not in EMISSIVITIES:
        raise ValueError(f"line profile: emissivity {emissivity!r} ('powerlaw' or 'texture')")
    if orders not in ORDERS:
        raise ValueError(f"line profile: orders {orders!r} ('first' or 'all')")
    if (r_inner is None) != (r_outer is None):
        raise ValueError("line profile: r_inner and r_outer come together (neither: the disk's annulus)")
    if r_inner is not None and not 0.0 < float(r_inner) < float(r_outer):
        raise ValueError(f"line profile: annulus ({r_inner}, {r_outer}): 0 < r_inner < r_outer")
    return dict(n_bins=int(n_bins), g_range=(g_min, g_max), index=float(index), power=float(power), emissivity=emissivity, orders=orders,
                r_inner=None if r_inner is None else float(r_inner), r_outer=None if r_outer is None else float(r_outer))


def unit_of(power: float) -> np.float32:
    """2^32 / 1.5^p in binary64, rounded once: the factor between a weight and its integer."""
    return np.float32(4294967296.0 / (G_CAP ** float(power)))


def scale_of(n_bins: int, g_range) -> np.float32:
    """n_bins / (g_max - g_min) on the f32 range in binary64, rounded once: the factor between g - g_min and a bin."""
    g_min, g_max = np.float32(g_range[0]), np.float32(g_range[1])
    return np.float32(float(n_bins) / (float(g_max) - float(g_min)))


def edges_of(n_bins: int, g_range) -> np.ndarray:
    """The n_bins + 1 bin edges in binary64."""
    g_min, g_max = float(np.float32(g_range[0])), float(np.float32(g_range[1]))
    return g_min + (g_max - g_min) * np.arange(int(n_bins) + 1, dtype=np.float64) / float(n_bins)


def flux_of(counts, power: float, g_range) -> np.ndarray:
    """Device integers (..., n_bins) -> flux per unit g: Q / unit / bin width, binary64."""
    counts = np.asarray(counts)
    n_bins = counts.shape[-1]
    width = (float(np.float32(g_range[1])) - float(np.float32(g_range[0]))) / n_bins
    return counts.astype(np.float64) / float(unit_of(power)) / width


def moments(edges, counts) -> dict:
    """g_mean (the flux-weighted mean of the bin centres) and g_red / g_blue (the lower edge of the lowest and the upper edge
    of the highest non-empty bin); NaN for an empty profile.  counts (n_bins,) or (n_frames, n_bins): one value or one per row."""
    edges = np.asarray(edges, dtype=np.float64)
    c = np.asarray(counts).astype(np.float64)
    rows = np.atleast_2d(c)
    centres = 0.5 * (edges[:-1] + edges[1:])
    total = rows.sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(total > 0, (rows * centres).sum(-1) / total, np.nan)
    red = np.full(rows.shape[0], np.nan)
    blue = np.full(rows.shape[0], np.nan)
    for k, row in enumerate(rows):
        nz = np.nonzero(row)[0]
        if nz.size:
            red[k], blue[k] = edges[nz[0]], edges[nz[-1] + 1]
    if c.ndim == 1:
        return dict(g_mean=float(mean[0]), g_red=float(red[0]), g_blue=float(blue[0]))
    return dict(g_mean=mean, g_red=red, g_blue=blue)


def profile(counts, under, over, settings: dict, spin: float, redshift: str, energy_kev: float = DEFAULT_ENERGY_KEV) -> dict:
    """What HipRenderer.kerr_line() returns and the .npz holds: edges, flux, counts, under, over, the moments, energy = g E0 at
    the bin centres, spin, redshift and the settings."""
    counts = np.asarray(counts, dtype=np.uint64)
    edges = edges_of(counts.shape[-1], settings["g_range"])
    out = dict(edges=edges, flux=flux_of(counts, settings["power"], settings["g_range"]), counts=counts,
               under=np.asarray(under, dtype=np.uint64), over=np.asarray(over, dtype=np.uint64))
    out.update(moments(edges, counts))
    out["energy"] = 0.5 * (edges[:-1] + edges[1:]) * float(energy_kev)
    out["energy_kev"] = float(energy_kev)
    out["spin"] = float(spin)
    out["redshift"] = str(redshift)
    out["settings"] = dict(settings)
    return out


def save_npz(path: str, prof: dict) -> None:
    """The profile as an .npz: every array and number of `prof`, the settings flattened (g_min, g_max, n_bins, index, power,
    emissivity, orders, r_inner, r_outer; NaN for an annulus left to the disk's)."""
    if not str(path).endswith(".npz"):
        raise ValueError(f"line profile: {path!r} is not an .npz path")
    s = prof["settings"]
    flat = {k: v for k, v in prof.items() if k != "settings"}
    flat.update(n_bins=s["n_bins"], g_min=s["g_range"][0], g_max=s["g_range"][1], index=s["index"], power=s["power"],
                emissivity=s["emissivity"], orders=s["orders"], r_inner=np.nan if s["r_inner"] is None else s["r_inner"],
                r_outer=np.nan if s["r_outer"] is None else s["r_outer"])
    with open(path, "wb") as f:
        np.savez(f, **flat)


def first_g(g_planes) -> np.ndarray:
    """The g of each pixel's first counted record from the (K, H, W) g planes (0 where a record does not count): (H, W), 0 where
    no record of the pixel counts."""
    g = np.asarray(g_planes, dtype=np.float32)
    hit = g != 0
    k = np.argmax(hit, axis=0)
    return np.where(hit.any(axis=0), np.take_along_axis(g, k[None], axis=0)[0], np.float32(0))


def g_colors(g, g_lo: float = 0.0, g_hi: float = G_CAP) -> np.ndarray:
    """The redshift map's colours, (..., 3) uint8: a scale that diverges about g = 1 -- white at 1, towards saturated red as g
    falls to g_lo, towards saturated blue as it rises to g_hi, each side monotone in g -- and black where g is 0, negative or
    not a number (nothing counted)."""
    g = np.asarray(g, dtype=np.float64)
    ok = np.isfinite(g) & (g > 0)
    gg = np.where(ok, g, 1.0)
    red_t = np.clip((1.0 - gg) / (1.0 - g_lo), 0.0, 1.0)      # 0 at g = 1, 1 at g_lo
    blue_t = np.clip((gg - 1.0) / (g_hi - 1.0), 0.0, 1.0)     # 0 at g = 1, 1 at g_hi
    r = 1.0 - blue_t
    gch = 1.0 - np.maximum(red_t, blue_t)
    b = 1.0 - red_t
    rgb = np.stack([r, gch, b], axis=-1)
    rgb = np.where(ok[..., None], rgb, 0.0)
    return np.floor(rgb * 255.0 + 0.5).astype(np.uint8)


def save_g_map(path: str, g_planes) -> None:
    """The redshift map of a frame as a PNG, written with the project's own PNG writer."""
    if not str(path).endswith(".png"):
        raise ValueError(f"redshift map: {path!r} is not a .png path")
    from .output import png_write
    png_write(path, np.ascontiguousarray(g_colors(first_g(g_planes))))
