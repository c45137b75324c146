"""TEST INFRASTRUCTURE -- NumPy restatement of the reference's lens flare (render.py:3925-4028),
pinned bit for bit by tests/golden/misc.npz and tests/golden/flare_cases.npz (generated from the
reference's _apply_lens_flare; tests/test_flare_ref.py).  The product path is the device kernel in csrc/flare.hip; only tests/ may import this module.


The reference works on (W, H, 3) arrays; frames here are (H, W, 3).  The effect is evaluated
on a (W, H, 3) copy so that every reduction runs over the same memory order as the reference
and the result is reproducible against its output.
"""
from __future__ import annotations

import numpy as np

_GHOST_TINT = np.array([1.0, 0.9, 0.7])
_RING_TINTS = (np.array([0.3, 0.4, 1.0]), np.array([0.5, 0.5, 0.9]), np.array([0.7, 0.5, 0.8]))
_HEX_TINT = np.array([0.6, 0.7, 1.0])
_STREAK_TINT = np.array([1.0, 0.95, 0.9])


def _flare_term_wh(disk: np.ndarray, probe: dict = None):
    """disk: (W, H, 3).  The f32 flare plane (W, H, 3) before it is added and clipped, None where the disk layer's total is
    under the threshold.  probe: a dict that receives what the tests' premises look at and the result does not show -- each
    shape's own alpha plane ("ghost0" .. "ghost7", "ring0" .. "ring2", "hex", "streaks": how many of the four wedges a pixel
    is in), the streaks' "delta" per axis, "total", "ratio" (total / (0.3 w h), as compared with 1.0) and "src"."""
    w, h, _ = disk.shape
    scale = min(w, h) / 360.0                      # sizes are quoted for a 360-line frame

    glow = np.max(disk, axis=2)                    # per-pixel disk brightness, (W, H)
    total = np.sum(glow)
    if probe is not None:
        probe["total"] = total
    if total < 0.01:
        return None
    xs, ys = np.mgrid[0:w, 0:h]
    src_x = np.sum(xs * glow) / total              # brightness centroid of the disk layer
    src_y = np.sum(ys * glow) / total
    mid_x, mid_y = w / 2, h / 2
    strength = min(total / (w * h * 0.3), 1.0) * 1.5
    if probe is not None:
        probe["ratio"], probe["src"] = total / (w * h * 0.3), (src_x, src_y)

    def along_axis(t):
        """Point at fraction t on the line source -> screen centre."""
        return src_x + (mid_x - src_x) * t, src_y + (mid_y - src_y) * t

    flare = np.zeros((w, h, 3), dtype=np.float32)

    # eight ghosts marching towards the centre, quadratic falloff
    for g in range(8):
        gx, gy = along_axis((g + 1) * 0.15)
        radius = (25 + g * 30) * scale
        dist = np.sqrt((xs - gx) ** 2 + (ys - gy) ** 2)
        inside = dist < radius
        alpha = np.zeros((w, h), dtype=np.float32)
        alpha[inside] = (1 - dist[inside] / radius) ** 2 * (1 - g * 0.08) * strength
        for c in range(3):
            flare[:, :, c] += alpha * _GHOST_TINT[c]
        if probe is not None:
            probe[f"ghost{g}"] = alpha

    # three diffraction rings with slightly different tints
    for k in range(3):
        rx, ry = along_axis(0.35 + k * 0.15)
        ring_r = (60 + k * 40) * scale
        ring_w = (6 + k * 3) * scale
        dist = np.sqrt((xs - rx) ** 2 + (ys - ry) ** 2)
        off = np.abs(dist - ring_r)
        alpha = np.clip(1 - off / ring_w, 0, 1) ** 2 * 0.5 * strength * (1 - k * 0.25)
        for c in range(3):
            flare[:, :, c] += alpha * _RING_TINTS[k][c]
        if probe is not None:
            probe[f"ring{k}"] = alpha

    # hexagonal aperture ring half way
    hx, hy = along_axis(0.5)
    dx, dy = xs - hx, ys - hy
    angle = np.arctan2(dy, dx)
    dist = np.sqrt(dx ** 2 + dy ** 2)
    edge = np.abs(np.mod(angle, np.pi / 3) - np.pi / 6)
    facet = np.clip(1 - edge / 0.2, 0, 1)
    off = np.abs(dist - 100 * scale)
    alpha = np.clip(1 - off / (15 * scale), 0, 1) ** 2 * facet * 0.3 * strength
    for c in range(3):
        flare[:, :, c] += alpha * _HEX_TINT[c]
    if probe is not None:
        probe["hex"] = alpha

    # four streaks through the source
    reach = min(w, h) * 0.4
    gain = strength * 0.3
    dx, dy = xs - src_x, ys - src_y
    dist = np.sqrt(dx ** 2 + dy ** 2)
    angle = np.arctan2(dy, dx)
    if probe is not None:
        probe["streaks"], probe["delta"] = np.zeros((w, h), dtype=np.int64), []
    for axis in [0, np.pi / 2, np.pi, 3 * np.pi / 2]:
        delta = np.abs(np.mod(angle - axis + np.pi, 2 * np.pi) - np.pi)
        on = delta < 0.05
        falloff = np.exp(-dist / reach)
        for c in range(3):
            flare[:, :, c] += np.where(on, falloff * gain * _STREAK_TINT[c], 0)
        if probe is not None:
            probe["streaks"] += on
            probe["delta"].append(delta)
    return flare


def _flare_wh(final: np.ndarray, disk: np.ndarray) -> np.ndarray:
    """final, disk: (W, H, 3).  Returns clip(final + flare, 0, 1)."""
    flare = _flare_term_wh(disk)
    if flare is None:
        return final
    return np.clip(final + flare, 0, 1)


def flare_term(disk_hw3: np.ndarray, probe: dict = None):
    """(H, W, 3) disk layer -> the (H, W, 3) f32 flare plane before it is added to the frame and clipped, or None where the
    layer's total is under the threshold and the frame stays untouched.  probe: see _flare_term_wh; its planes are (W, H)."""
    flare = _flare_term_wh(np.ascontiguousarray(disk_hw3.transpose(1, 0, 2)), probe)
    return None if flare is None else np.ascontiguousarray(flare.transpose(1, 0, 2))


def apply_lens_flare(final_hw3: np.ndarray, disk_hw3: np.ndarray) -> np.ndarray:
    """(H, W, 3) frame + (H, W, 3) disk layer -> (H, W, 3) frame with the flare added."""
    final = np.ascontiguousarray(final_hw3.transpose(1, 0, 2))
    disk = np.ascontiguousarray(disk_hw3.transpose(1, 0, 2))
    out = _flare_wh(final, disk)
    return np.ascontiguousarray(out.transpose(1, 0, 2))
