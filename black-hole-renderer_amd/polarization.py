"""Polarisation of the disk: field presets, the checks of its three numbers, and what the host does with Stokes planes.

The device computes Stokes I, Q, U per pixel of a frame from the ray map (HipRenderer.set_polarization, include/bhr.h
"polarisation") and their means over cells.  Here: the field's presets, ``check``, ``degree_and_angle``, the tick overlay drawn
from cell means of Q and U (angles are never averaged), and the .npz a still or a video writes.

Convention: the electric-vector position angle chi = atan2(U, Q) / 2 is counted from image-right towards image-up.  The IAU
convention counts it from north (image-up) through east (image-LEFT on the sky): chi_IAU = chi - pi / 2, that is
Q_IAU = -Q and U_IAU = -U.
"""
from __future__ import annotations

import numpy as np

PRESETS = {"toroidal": (0.0, 1.0, 0.0), "radial": (1.0, 0.0, 0.0), "vertical": (0.0, 0.0, 1.0)}
DEFAULT_FRACTION = 0.7
DEFAULT_CELL = 16
CELLS = (8, 16, 32)
CONVENTION = ("chi = atan2(U, Q) / 2 from image-right towards image-up; IAU (from north through east): Q_IAU = -Q, U_IAU = -U")


def field_vector(field):
    """A preset's name, or three numbers (b_r, b_phi, b_z) in the gas frame -> a tuple of three floats.  ValueError for an
    unknown name, another count, a component that is not finite, or the zero field."""
    if isinstance(field, str):
        if field not in PRESETS:
            raise ValueError(f"polarization field {field!r}: one of {sorted(PRESETS)} or three numbers BR BPHI BZ")
        return PRESETS[field]
    try:
        b = tuple(float(v) for v in field)
    except (TypeError, ValueError):
        raise ValueError(f"polarization field {field!r}: one of {sorted(PRESETS)} or three numbers BR BPHI BZ") from None
    if len(b) != 3:
        raise ValueError(f"polarization field takes three numbers BR BPHI BZ, got {len(b)}")
    if not all(np.isfinite(b)) or not any(v != 0.0 for v in b):
        raise ValueError(f"polarization field {b}: finite and not zero")
    return b


def parse_field(tokens):
    """The command line's --polarization FIELD: one token naming a preset, or three numbers."""
    tokens = list(tokens)
    if len(tokens) == 1:
        try:
            float(tokens[0])
        except ValueError:
            return field_vector(tokens[0])
    return field_vector(tokens)


def check(field, fraction=DEFAULT_FRACTION, cell=DEFAULT_CELL) -> dict:
    """-> dict(field=(b_r, b_phi, b_z), fraction=, cell=), or ValueError naming what is wrong: the field (field_vector), a
    fraction outside [0, 1], a cell other than 8, 16 or 32."""
    b = field_vector(field)
    try:
        f = float(fraction)
    except (TypeError, ValueError):
        raise ValueError(f"polarization_fraction is a number in [0, 1], got {fraction!r}") from None
    if not 0.0 <= f <= 1.0:               # a NaN fails the comparison too
        raise ValueError(f"polarization_fraction is a number in [0, 1], got {fraction!r}")
    if cell not in CELLS or isinstance(cell, bool):
        raise ValueError(f"polarization_cell is one of {CELLS}, got {cell!r}")
    return {"field": b, "fraction": f, "cell": int(cell)}


def degree_and_angle(I, Q, U):
    """Degree of linear polarisation sqrt(Q^2 + U^2) / I (0 where I is 0) and the angle chi = atan2(U, Q) / 2 in radians,
    from image-right towards image-up."""
    I, Q, U = (np.asarray(v, dtype=np.float64) for v in (I, Q, U))
    p = np.hypot(Q, U)
    with np.errstate(divide="ignore", invalid="ignore"):
        deg = np.where(I > 0, p / np.where(I > 0, I, 1.0), 0.0)
    return deg, 0.5 * np.arctan2(U, Q)


def draw_ticks(rgb_u8, cells, cell, color=(255, 255, 255), scale=0.9) -> np.ndarray:
    """A copy of the (H, W, 3) uint8 frame with one line segment per cell of the (gh, gw, 3) grid of (I, Q, U) means: centred
    on the cell, its full length ``scale * cell * sqrt(Q^2 + U^2) / (Pi_max I_max)`` with I_max the largest cell mean of I and
    Pi_max the largest sqrt(Q^2 + U^2) / I_max of the grid (so the strongest tick spans ``scale`` of a cell), its orientation
    atan2(U, Q) / 2 from image-right towards image-up (rows grow downwards: the segment is drawn along (cos chi, -sin chi)).
    Plain NumPy rasterisation, a pixel per step of the longer axis."""
    out = np.array(rgb_u8, dtype=np.uint8, copy=True)
    cells = np.asarray(cells, dtype=np.float64)
    h, w = out.shape[:2]
    gh, gw = cells.shape[:2]
    i_max = float(cells[..., 0].max()) if cells.size else 0.0
    if not i_max > 0.0:
        return out
    pol = np.hypot(cells[..., 1], cells[..., 2]) / i_max
    p_max = float(pol.max())
    if not p_max > 0.0:
        return out
    for gy in range(gh):
        for gx in range(gw):
            half = 0.5 * scale * cell * pol[gy, gx] / p_max
            if not half >= 0.5:
                continue
            chi = 0.5 * np.arctan2(cells[gy, gx, 2], cells[gy, gx, 1])
            # the centre of the pixels the cell has (an edge cell is cut by the frame)
            cx = 0.5 * (gx * cell + min((gx + 1) * cell, w)) - 0.5
            cy = 0.5 * (gy * cell + min((gy + 1) * cell, h)) - 0.5
            dx, dy = half * np.cos(chi), -half * np.sin(chi)
            n = int(np.ceil(2.0 * max(abs(dx), abs(dy)))) + 1
            t = np.linspace(-1.0, 1.0, n)
            xs = np.rint(cx + t * dx).astype(np.int64)
            ys = np.rint(cy + t * dy).astype(np.int64)
            ok = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
            out[ys[ok], xs[ok]] = color
    return out


def write_stokes(path, cells, cell, field, fraction, camera=None, stokes=None, hole=None) -> None:
    """A compressed .npz: ``cells`` -- (gh, gw, 3) of a still or (n_frames, gh, gw, 3) of a video --, ``cell``, ``field``,
    ``fraction``, ``convention`` (CONVENTION), ``cam_pos`` / ``fov`` where ``camera`` = dict(cam_pos=, fov=) is given, and
    where ``stokes`` (3, H, W) is given the planes ``I``, ``Q``, ``U`` (a still; a video carries the grids only); with ``hole`` =
    dict(spin=, redshift=) -- the Kerr polarisation's files -- also ``spin`` (a / M) and ``redshift`` ("model" or "exact")."""
    if not str(path).lower().endswith(".npz"):
        raise ValueError(f"the Stokes output is written as a .npz file, got {path!r}")
    data = {"cells": np.asarray(cells, dtype=np.float32), "cell": np.int32(cell), "field": np.asarray(field_vector(field), dtype=np.float64),
            "fraction": np.float64(fraction), "convention": np.array(CONVENTION)}
    if camera is not None:
        data["cam_pos"] = np.asarray(camera["cam_pos"], dtype=np.float64)
        data["fov"] = np.float64(camera["fov"])
    if hole is not None:
        data["spin"] = np.float64(hole["spin"])
        data["redshift"] = np.array(str(hole["redshift"]))
    if stokes is not None:
        s = np.asarray(stokes, dtype=np.float32)
        data["I"], data["Q"], data["U"] = s[0], s[1], s[2]
    with open(path, "wb") as fh:
        np.savez_compressed(fh, **data)
