"""CPU reference of the Kerr camera (include/bhr.h: bhr_render_kerr_view; DESIGN.md "Kerr camera"), in NumPy.

Imports nothing from the product.  It is put together from the references of its halves:
    tests/projection_ref.py     the equirectangular and fisheye pixel directions n' (the pinhole's are kerr_ref.pixel_rays)
    tests/observer_ref.py       aberration (n' -> n, D) and the sky under D
    tests/kerr_ref.py           the Kerr march from n, the samplers, the model g-factor
    tests/kerr_redshift_ref.py  the march that keeps the photon at a crossing, the exact g-factor, the shade from g on
and states only what is new: D is a factor of g ahead of its cap, in this product order:
    model   g = min((g_doppler (grav_num / grav_den)) D, 1.5)
    exact   g = min((nu_obs D) / max(nu_em, 1e-3), 1.5)
and on the sky sample under sky_shift (observer_ref.sky_shift), ahead of the product with 1 - alpha.  A fisheye pixel outside
the image circle has no ray: BG and DISK exactly 0, no step.  binary64 by default, dtype=np.float32 operation by operation in f32.

The named velocities are restated from the 4 x 4 Kerr-Schild metric (velocity() below), not from the product's closed form.
"""
import numpy as np

import kerr_redshift_ref as X
import kerr_ref as K
import observer_ref as R
import projection_ref as P

M = K.M


# ----------------------------------------------------------------------------------------------- named velocities
def ks_metric(pos, A):
    """g_{mu nu} = eta + f l l at `pos`, binary64, of the hole that turns in the DISK's sense (clockwise seen from +z, v_hat =
    r_hat x z_hat) for A > 0: the ingoing Kerr-Schild form, whose hole turns counter-clockwise for a' > 0, with a' = -A M."""
    x, y, z = (float(v) for v in pos)
    a = -float(A) * M
    w = x * x + y * y + z * z - a * a
    S = np.sqrt(w * w + 4.0 * a * a * z * z)
    r = np.sqrt(0.5 * (w + S))
    f = r / S
    q = r * r + a * a
    l = np.array([1.0, (r * x + a * y) / q, (r * y - a * x) / q, z / r])
    return np.diag([-1.0, 1.0, 1.0, 1.0]) + f * np.outer(l, l)


def orbit_gamma(pos, A, omega):
    """gamma = -u.u_static of the camera at `pos` that circles the axis with angular velocity omega in the disk's sense."""
    g = ks_metric(pos, A)
    x, y, _ = (float(v) for v in pos)
    u = np.array([1.0, omega * y, -omega * x, 0.0])
    us = np.array([1.0, 0.0, 0.0, 0.0])
    return float(-(u @ g @ us) / np.sqrt(-(u @ g @ u)) / np.sqrt(-(us @ g @ us)))


def omega_of(kind, pos, A):
    """The angular velocity (disk's sense positive) of a named observer at `pos`: circular = Kerr's equatorial geodesic
    sqrt(M) / (r^1.5 + a sqrt(M)); zamo = the one whose u_phi vanishes, from the 4 x 4 metric: u_mu (d/dphi)^mu = 0."""
    x, y, z = (float(v) for v in pos)
    a = float(A) * M
    if kind == "circular":
        r = float(K.ks_radius(np.array([[x, y, z]]), a)[0])
        return np.sqrt(M) / (r ** 1.5 + a * np.sqrt(M))
    if kind == "zamo":
        g = ks_metric(pos, A)
        k = np.array([0.0, y, -x, 0.0])                  # d/dphi in the disk's sense
        t = np.array([1.0, 0.0, 0.0, 0.0])
        return float(-(t @ g @ k) / (k @ g @ k)) if x * x + y * y > 0 else 0.0
    raise ValueError(kind)


def velocity(kind, pos, A):
    """beta of the named observer as the static observer at `pos` measures it: sign(omega) sqrt(1 - 1 / gamma^2) v_hat."""
    if kind == "static":
        return np.zeros(3)
    x, y, _ = (float(v) for v in pos)
    rho = np.hypot(x, y)
    if rho == 0:
        return np.zeros(3)
    om = omega_of(kind, pos, A)
    if om == 0:
        return np.zeros(3)
    gam = orbit_gamma(pos, A, om)
    return np.sign(om) * np.sqrt(max(1.0 - 1.0 / (gam * gam), 0.0)) * np.array([y / rho, -x / rho, 0.0])


# ----------------------------------------------------------------------------------------------- g with D
def g_model(hx, hy, hit_r, to_cam, a, cam_pos, D):
    """kerr_ref.g_factor's g, statement by statement, with D ahead of the cap."""
    t = hx.dtype.type
    rs = t(K.RS)
    r_obs = np.sqrt((cam_pos.astype(hx.dtype) ** 2).sum())
    r_em = hit_r
    r_safe = np.maximum(r_em, rs + t(1e-3))
    omega = K.omega_kerr(r_safe, a)
    lorentz = np.sqrt(np.maximum(t(1) - rs / r_safe, t(1e-6)))
    beta = np.minimum(r_safe * omega / np.maximum(lorentz, t(1e-6)), t(0.99))
    gamma = t(1) / np.sqrt(np.maximum(t(1) - beta * beta, t(1e-6)))
    inv = t(1) / np.sqrt(hx * hx + hy * hy)
    rx, ry = inv * hx, inv * hy
    vx, vy = ry, -rx
    v_norm = np.sqrt(vx * vx + vy * vy)
    good = v_norm > t(1e-6)
    vn = np.where(good, v_norm, t(1))
    vx, vy = np.where(good, vx / vn, t(0)), np.where(good, vy / vn, t(1))
    ti = t(1) / np.sqrt((to_cam * to_cam).sum(-1))
    cos_theta = vx * (ti * to_cam[:, 0]) + vy * (ti * to_cam[:, 1])
    denom = np.maximum(t(1) - beta * cos_theta, t(1e-3))
    g_doppler = t(1) / (gamma * denom)
    grav_num = np.sqrt(np.maximum(t(1) - rs / np.maximum(r_obs, rs + t(1e-3)), t(1e-6)))
    grav_den = np.sqrt(np.maximum(t(1) - rs / np.maximum(r_em, rs + t(1e-3)), t(1e-6)))
    return np.minimum(g_doppler * (grav_num / grav_den) * D, t(K.G_FACTOR_CAP))


def g_exact(hx, hy, lz, Pr, U, a, cam_pos, isco, D):
    """kerr_redshift_ref.g_exact with the static observer's nu_obs turned into the moving one's."""
    t = hx.dtype.type
    r_isco, E, L = isco
    r = np.sqrt(hx * hx + hy * hy - t(a) * t(a))
    nu_c = X.nu_em_circular(r, a, lz, K.omega_kerr(r, a))
    with np.errstate(invalid="ignore", divide="ignore"):
        nu_p = X.nu_em_plunge(r, a, lz, Pr, U, r_isco, E, L)
    nu_em = np.where(r >= t(r_isco), nu_c, nu_p)
    return np.minimum(X.nu_observer(cam_pos, a, hx.dtype) * D / np.maximum(nu_em, t(X.NU_EM_MIN)), t(K.G_FACTOR_CAP))


# ----------------------------------------------------------------------------------------------- the frame
def render(cam, A, sky, tex, beta=None, sky_shift_on=True, projection=None, fov=None, redshift="model", h_base=0.1, r_inner=2.0,
           r_outer=15.0, t_offset=0.0, dtype=np.float64):
    """One frame of the Kerr camera `cam` (kerr_ref.build_camera) moving with beta (None: at rest with a plain sky), through the
    pinhole (projection None) or "equirect" / "fisheye" with fov in degrees.  kerr_ref.render's dict (bg, disk, final, fate,
    n_hits, steps, esc_dir, first_hit) and inside, D (H, W)."""
    if beta is None:
        beta, sky_shift_on = (0.0, 0.0, 0.0), False
    t = np.dtype(dtype).type
    K.check_camera(cam["pos"], A)
    W, H = cam["width"], cam["height"]
    if projection is None:
        npr, inside = K.pixel_rays(cam, dtype), np.ones((H, W), dtype=bool)
    else:
        npr, inside = P.directions(cam, projection, fov, dtype)
    live = np.nonzero(inside.reshape(-1))[0]
    d, D = R.aberrate(npr.reshape(-1, 3)[live], beta, dtype)
    exact = redshift == "exact"
    m = (X.march if exact else K.march)(cam["pos"].astype(dtype), d, A, h_base, cam["r_escape"], r_inner, r_outer, dtype)
    a = t(A) * t(M)
    isco = X.isco_orbit(A)
    n = live.size
    accum = np.zeros((n, 3), dtype=dtype)
    alpha = np.zeros(n, dtype=dtype)
    rows = m["hits"]
    first = np.full((n, 2), np.nan)
    for k in range(int(rows[:, 1].max()) + 1 if rows.shape[0] else 0):       # front to back
        sel = rows[rows[:, 1] == k]
        ray = sel[:, 0].astype(np.int64)
        hx, hy = sel[:, 2].astype(dtype), sel[:, 3].astype(dtype)
        if k == 0:
            first[ray] = sel[:, 2:4]
        hit_r = np.sqrt(hx * hx + hy * hy - a * a)
        if exact:
            g = g_exact(hx, hy, sel[:, 4].astype(dtype), sel[:, 5].astype(dtype), sel[:, 6].astype(dtype), a, cam["pos"], isco, D[ray])
        else:
            g = g_model(hx, hy, hit_r, sel[:, 4:7].astype(dtype), a, cam["pos"], D[ray])
        rgba = K.sample_disk(tex, hx, hy, hit_r, a, r_inner, r_outer, t_offset)
        base_alpha = np.minimum(rgba[:, 3], t(0.999))
        disk_alpha = t(1) - (t(1) - base_alpha) ** t(K.DISK_ALPHA_GAIN)
        col = X.shade_g(rgba[:, :3], g, hit_r, r_inner, r_outer)
        front = t(1) - alpha[ray]
        accum[ray] = accum[ray] + col * (disk_alpha * front)[:, None]
        alpha[ray] = t(1) - front * (t(1) - disk_alpha)
    bg = np.zeros((n, 3), dtype=dtype)
    esc = m["fate"] == 1
    if esc.any():
        c = K.sample_skybox(sky, m["esc_dir"][esc].astype(dtype))
        if sky_shift_on:
            c = R.sky_shift(c, D[esc])
        bg[esc] = c * (t(1) - alpha[esc])[:, None]
    disk = np.clip(accum, t(0), t(1))

    def frame(values, fill, shape, dt):                  # the live pixels' values in the frame, `fill` outside the image circle
        out = np.full((W * H,) + shape, fill, dtype=dt)
        out[live] = values
        return out.reshape((H, W) + shape)
    return dict(bg=frame(bg, 0, (3,), dtype), disk=frame(disk, 0, (3,), dtype), final=frame(np.clip(bg + disk, t(0), t(1)), 0, (3,), dtype),
                fate=frame(m["fate"], 2, (), np.int8), n_hits=frame(m["n_hits"], 0, (), np.int32), steps=frame(m["steps"], 0, (), np.int64),
                esc_dir=frame(np.where(esc[:, None], m["esc_dir"], 0.0), 0.0, (3,), np.float64), first_hit=frame(first, np.nan, (2,), np.float64),
                inside=inside, D=frame(D, 1, (), dtype))
