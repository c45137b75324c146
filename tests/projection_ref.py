"""CPU reference of the projections (include/bhr.h: bhr_render_projected; DESIGN.md "Projections"), in NumPy.

Imports nothing from the product.  The two direction formulas are restated here, in binary64 by default and with
dtype=np.float32 operation by operation in f32 (NumPy's sin and cos stand in for the device library's: their bits are not
pinned); everything behind the direction -- aberration, the Schwarzschild march, the g-factor, the samplers -- is
tests/observer_ref.py's.  A fisheye pixel outside the image circle has no ray: BG and DISK exactly 0, no step.
"""
import numpy as np

import kerr_ref as K
import observer_ref as R

EQUIRECT, FISHEYE = "equirect", "fisheye"


def spans(kind, fov, dtype=np.float64):
    """(span_h, span_v) in radians as the march takes them: binary64, rounded once to dtype.  Equirect: the two spans; fisheye:
    HALF the full angle, and 0."""
    t = np.dtype(dtype).type
    if kind == EQUIRECT:
        return t(np.radians(np.float64(np.float32(fov[0])))), t(np.radians(np.float64(np.float32(fov[1]))))
    return t(np.radians(np.float64(np.float32(fov[0]))) / 2.0), t(0)


def pixel_coefficients(kind, fov, width, height, dtype=np.float64):
    """(a, b, c, inside), each (H, W): n' = a F + b R + c U and the fisheye's mask (all True for equirect)."""
    t = np.dtype(dtype).type
    W, H = int(width), int(height)
    px = (np.arange(W, dtype=dtype) + t(0.5))[None, :]
    py = (np.arange(H, dtype=dtype) + t(0.5))[:, None]
    span_h, span_v = spans(kind, fov, dtype)
    if kind == EQUIRECT:
        lon = np.broadcast_to((px / t(W) - t(0.5)) * span_h, (H, W))
        lat = np.broadcast_to((t(0.5) - py / t(H)) * span_v, (H, W))
        cl = np.cos(lat)
        return (cl * np.cos(lon)).astype(dtype), (cl * np.sin(lon)).astype(dtype), np.sin(lat).astype(dtype), np.ones((H, W), dtype=bool)
    if kind != FISHEYE:
        raise ValueError(kind)
    s = t(2) / t(min(W, H))
    x = np.broadcast_to((px - t(W) / t(2)) * s, (H, W))
    y = np.broadcast_to((t(H) / t(2) - py) * s, (H, W))
    rho = np.sqrt(x * x + y * y)
    inside = rho <= t(1)
    theta = rho * span_h
    with np.errstate(divide="ignore"):
        inv = np.where(rho > 0, t(1) / np.where(rho > 0, rho, t(1)), t(0)).astype(dtype)
    st = np.sin(theta)
    return np.cos(theta).astype(dtype), (st * (x * inv)).astype(dtype), (st * (y * inv)).astype(dtype), inside


def directions(cam, kind, fov, dtype=np.float64):
    """(n' (H, W, 3), inside (H, W)) of the camera `cam` (kerr_ref.build_camera: its basis and frame size; pw, ph unused)."""
    a, b, c, inside = pixel_coefficients(kind, fov, cam["width"], cam["height"], dtype)
    F, Rt, U = (cam[k].astype(dtype) for k in ("forward", "right", "up"))
    n = np.stack([(a * F[k] + b * Rt[k]) + c * U[k] for k in range(3)], axis=-1)
    return n.astype(dtype), inside


def render(cam, kind, fov, beta, sky, tex, h_base=0.1, r_inner=2.0, r_outer=15.0, tilt_deg=0.0, t_offset=0.0, sky_shift_on=True, dtype=np.float64):
    """One projected frame of `cam` moving with beta (None: at rest with a plain sky): observer_ref.render with the pixel
    directions replaced.  dict with bg, disk (H, W, 3) in dtype, fate, n_hits, steps (H, W), inside (H, W), D and n."""
    if beta is None:
        beta, sky_shift_on = (0.0, 0.0, 0.0), False
    t = np.dtype(dtype).type
    W, H = cam["width"], cam["height"]
    npr, inside = directions(cam, kind, fov, dtype)
    live = np.nonzero(inside.reshape(-1))[0]             # the pixels that have a ray; the rest keep their zeros
    n_dir, D = R.aberrate(npr.reshape(-1, 3)[live], beta, dtype)
    m = R.march(cam["pos"].astype(dtype), n_dir, h_base, cam["r_escape"], r_inner, r_outer, tilt_deg, dtype)
    tilt = np.float32(np.float32(tilt_deg) * np.float32(np.pi) / np.float32(180.0)).astype(dtype)
    tan_t, sin_t, cos_t = t(np.tan(tilt)), t(np.sin(tilt)), t(np.cos(tilt))
    n = live.size
    accum = np.zeros((n, 3), dtype=dtype)
    alpha = np.zeros(n, dtype=dtype)
    rows = m["hits"]
    for k in range(int(rows[:, 1].max()) + 1 if rows.shape[0] else 0):       # front to back, as observer_ref.render shades
        sel = rows[rows[:, 1] == k]
        ray = sel[:, 0].astype(np.int64)
        hx, hy, to_cam = sel[:, 2].astype(dtype), sel[:, 3].astype(dtype), sel[:, 4:7].astype(dtype)
        hit_r = np.sqrt(hx * hx + hy * hy)
        rgba = K.sample_disk(tex, hx, hy, hit_r, 0.0, r_inner, r_outer, t_offset)
        base_alpha = np.minimum(rgba[:, 3], t(0.999))
        disk_alpha = t(1) - (t(1) - base_alpha) ** t(K.DISK_ALPHA_GAIN)
        col = R.g_factor(rgba[:, :3], hx, hy, hy * tan_t, hit_r, to_cam, cam["pos"], r_inner, r_outer, sin_t, cos_t, D[ray])
        front = t(1) - alpha[ray]
        accum[ray] = accum[ray] + col * disk_alpha[:, None] * front[:, None]
        alpha[ray] = t(1) - front * (t(1) - disk_alpha)
    bg = np.zeros((n, 3), dtype=dtype)
    esc = m["fate"] == 1
    if esc.any():
        e = m["esc_dir"][esc].astype(dtype)
        e = (t(1) / np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]))[:, None] * e
        c = K.sample_skybox(sky, e)
        if sky_shift_on:
            c = R.sky_shift(c, D[esc])
        bg[esc] = c * (t(1) - alpha[esc])[:, None]

    def frame(values, fill, shape, dt):                  # the live pixels' values in the frame, `fill` outside the image circle
        out = np.full((W * H,) + shape, fill, dtype=dt)
        out[live] = values
        return out.reshape((H, W) + shape)
    return dict(bg=frame(bg, 0, (3,), dtype), disk=frame(np.clip(accum, t(0), t(1)), 0, (3,), dtype), fate=frame(m["fate"], 2, (), np.int8),
                n_hits=frame(m["n_hits"], 0, (), np.int32), steps=frame(m["steps"], 0, (), np.int64), inside=inside,
                D=frame(D, 1, (), dtype), n=frame(n_dir, 0, (3,), dtype), n_prime=npr)
