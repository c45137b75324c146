"""Point stars: the star catalogue a ray map's frames render as lensed points (HipRenderer.set_stars; include/bhr.h states the
model, DESIGN 4 "Point stars").

A star is a unit direction on the celestial sphere -- in the sky's own convention, theta = acos(u.z), phi = atan2(u.y, u.x), as
the march's skybox sampler takes a direction -- and an RGB flux in units of sky value x steradian.  ``catalog_from_tables``
makes the catalogue of the procedural sky from the tables its texture is rasterised from, ``starless_tables`` the same tables
without the baked blobs, ``bin_catalog`` the equirectangular grid the device looks stars up in (the library bins on its own;
this is its host twin, for tests and tools).
"""
from __future__ import annotations

import numpy as np

DEFAULT_MAX_MAGNIFICATION = 32.0
DEFAULT_MAX_SPAN_DEG = 10.0
DEFAULT_STAR_GAIN = 2.0
MAX_STARS = 1 << 22


def catalog_from_tables(tables: dict, gain: float, pixel_solid_angle: float):
    """The procedural catalogue of ``skybox.sky_tables``: (dirs (n, 3) float64 unit vectors, flux (n, 3) float64).

    A star sits where its blob's centre texel is sampled: phi = cx / tex_w 2 pi, theta = cy / tex_h pi, in binary64 from the
    tables' float32 cx, cy.  Phi = gain * colour * brightness * pixel_solid_angle, brightness the blob's centre value: an
    unlensed star deposits gain * brightness * colour in total on a frame whose pixel has that solid angle."""
    if not (gain > 0 and np.isfinite(gain)):
        raise ValueError(f"catalog_from_tables: gain {gain!r} (above 0)")
    if not (pixel_solid_angle > 0 and np.isfinite(pixel_solid_angle)):
        raise ValueError(f"catalog_from_tables: pixel_solid_angle {pixel_solid_angle!r} (above 0)")
    cx = np.asarray(tables["cx"], dtype=np.float64)
    cy = np.asarray(tables["cy"], dtype=np.float64)
    phi = cx / float(tables["tex_w"]) * (2.0 * np.pi)
    theta = cy / float(tables["tex_h"]) * np.pi
    dirs = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=-1)
    dx, dy = np.asarray(tables["dx"]), np.asarray(tables["dy"])
    centre = int(np.flatnonzero((dx == 0) & (dy == 0))[0])
    brightness = np.asarray(tables["vals"], dtype=np.float64)[:, centre]
    flux = float(gain) * np.asarray(tables["colors"], dtype=np.float64) * brightness[:, None] * float(pixel_solid_angle)
    return dirs, flux


def starless_tables(tables: dict) -> dict:
    """The same tables with the blob values zeroed: the nebula (and, rasterised with the glow, the Milky Way) stay the
    reference's texture, without the baked stars."""
    out = dict(tables)
    out["vals"] = np.zeros_like(np.asarray(tables["vals"]))
    return out


def grid_shape(n: int):
    """(bins_theta, bins_phi) for n stars: about 8 stars per bin, twice as many bins in longitude (the library's rule)."""
    t = int(min(max(int(np.floor(np.sqrt(n / 16.0) + 0.5)), 4), 256))
    return t, 2 * t


def bin_catalog(dirs, bins_theta: int = 0, bins_phi: int = 0):
    """Sort a catalogue into the equirectangular grid: (offsets (bins + 1,) int32, order (n,) int32) -- bin b = t * bins_phi + p
    holds the stars order[offsets[b]:offsets[b + 1]], in catalogue order.  The bin of a direction is taken from its float32
    rounding in binary64: t = floor(acos(z) / pi * bins_theta), p = floor(phi / (2 pi) * bins_phi) with phi in [0, 2 pi), both
    clamped into the grid."""
    d = np.asarray(dirs, dtype=np.float64)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32).astype(np.float64)
    n = len(d)
    if not bins_theta:
        bins_theta, bins_phi = grid_shape(max(n, 1))
    theta = np.arccos(np.clip(d[:, 2], -1.0, 1.0))
    phi = np.arctan2(d[:, 1], d[:, 0])
    phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
    t = np.clip(np.floor(theta / np.pi * bins_theta).astype(np.int64), 0, bins_theta - 1)
    p = np.clip(np.floor(phi / (2.0 * np.pi) * bins_phi).astype(np.int64), 0, bins_phi - 1)
    b = t * bins_phi + p
    order = np.argsort(b, kind="stable").astype(np.int32)
    offsets = np.zeros(bins_theta * bins_phi + 1, dtype=np.int32)
    np.cumsum(np.bincount(b, minlength=bins_theta * bins_phi), out=offsets[1:])
    return offsets, order


def check_catalog(dirs, flux):
    """(dirs, flux) as contiguous float32 (n, 3) arrays, as the C ABI takes them (the library normalizes the directions in
    binary64 and rounds them once), after the checks of bhr_set_stars that need no context."""
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(flux, dtype=np.float64).reshape(-1, 3)
    if len(d) != len(f):
        raise ValueError(f"set_stars: {len(d)} directions for {len(f)} fluxes")
    if len(d) > MAX_STARS:
        raise ValueError(f"set_stars: {len(d)} stars (0 .. {MAX_STARS})")
    norm = np.linalg.norm(d, axis=-1)
    if len(d) and not (np.all(np.isfinite(d)) and np.all(np.abs(norm - 1.0) <= 1e-3)):
        raise ValueError("set_stars: a direction is not finite or not a unit vector (within 1e-3)")
    if len(f) and not (np.all(np.isfinite(f)) and np.all(f >= 0)):
        raise ValueError("set_stars: a flux is negative or not finite")
    return np.ascontiguousarray(d, dtype=np.float32), np.ascontiguousarray(f, dtype=np.float32)
