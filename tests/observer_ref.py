"""CPU reference of the moving observer (include/bhr.h: bhr_render_observer; DESIGN.md "Observer"), in NumPy.

Imports nothing from the product.  The sky and disk samplers, the camera and the step factor are tests/kerr_ref.py's (at a = 0
they are the Schwarzschild ones); the Schwarzschild march is restated here: d2x/dl2 = -1.5 L^2 x / r^5 with L = |d x p| of the
launch, RK4, the reference's dt_fac, capture at r < r_s, escape beyond r_escape or the affine limit, and the interpolated
crossing of the plane z - y tan(tilt) with the hit's x and y.  The g-factor is restated too, because it takes the disk's tilt
and the observer's D ahead of its cap.  binary64 by default; dtype=np.float32 evaluates every operation in f32, in the order the
device's strict arithmetic has them (the exactly rounded sqrt and divide are NumPy's).

Units r_s = 1, M = 1/2.  beta is the camera's velocity as the static observer at its position measures it, in units of c.
"""
import numpy as np

import kerr_ref as K

RS = 1.0
BETA_MAX = 0.995


# ----------------------------------------------------------------------------------------------- the observer
def gamma_of(beta):
    b = np.asarray(beta, dtype=np.float64)
    return 1.0 / np.sqrt(1.0 - float(b @ b))


def aberrate(n_prime, beta, dtype=np.float64):
    """(n, D): the static-frame direction of the ray whose direction in the moving camera's frame is n_prime (..., 3), and
    D = nu_observed / nu_static.  gamma and gamma^2 / (gamma + 1) in binary64 rounded once to dtype; the rest in dtype:
      D = 1 / (gamma (1 - beta.n')),  n = (n' + (gamma^2 / (gamma + 1)) (beta.n') beta - gamma beta) D   (not renormalised)"""
    t = np.dtype(dtype).type
    b = np.asarray(beta, dtype=np.float32).astype(dtype)       # the velocity travels as three f32; gamma is made of those
    g64 = gamma_of(b)
    g, g2 = t(g64), t(g64 * g64 / (g64 + 1.0))
    npr = np.asarray(n_prime, dtype=dtype)
    bn = (b[0] * npr[..., 0] + b[1] * npr[..., 1]) + b[2] * npr[..., 2]
    D = t(1) / (g * (t(1) - bn))
    c = g2 * bn
    n = np.stack([((npr[..., k] + c * b[k]) - g * b[k]) * D for k in range(3)], axis=-1)
    return n.astype(dtype), D.astype(dtype)


def boost_forward(n, beta):
    """The direction in the moving frame of a ray whose static-frame direction is n (binary64): the inverse of aberrate."""
    b = np.asarray(beta, dtype=np.float32).astype(np.float64)  # as aberrate takes it
    g = gamma_of(b)
    n = np.asarray(n, dtype=np.float64)
    bn = n @ b
    return (n + ((g * g / (g + 1.0)) * bn)[..., None] * b + g * b) / (g * (1.0 + bn))[..., None]


def velocity(kind, pos):
    """The named velocities (binary64), restated: static 0; circular sqrt(0.5 / (r - 1)) normalize(r_hat x z_hat); infall
    -sqrt(1 / r) r_hat."""
    p = np.asarray(pos, dtype=np.float64)
    r = np.linalg.norm(p)
    if kind == "static":
        return np.zeros(3)
    if kind == "circular":
        t = np.cross(p / r, [0.0, 0.0, 1.0])
        return np.sqrt(0.5 / (r - 1.0)) * t / np.linalg.norm(t)
    if kind == "infall":
        return -np.sqrt(1.0 / r) * p / r
    raise ValueError(kind)


def sky_shift(c, D):
    """The sky sample under the observer's Doppler factor: c (r_s I, I, b_s I)."""
    t = D.dtype.type
    Ds = np.clip(D, t(0.1), t(K.G_FACTOR_CAP))
    I = Ds ** t(K.G_LUMINOSITY_POWER)
    w = t(1) - t(1) / Ds
    g_s = np.exp(t(2.72) * w)
    r_s = np.minimum(np.exp(t(2.21) * w) / g_s, t(3))
    b_s = np.minimum(np.exp(t(3.13) * w) / g_s, t(3))
    return np.stack([c[:, 0] * (r_s * I), c[:, 1] * I, c[:, 2] * (b_s * I)], axis=-1)


# ----------------------------------------------------------------------------------------------- the Schwarzschild march
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def march(x0, d, h_base=0.1, r_escape=12.0, r_inner=2.0, r_outer=15.0, tilt_deg=0.0, dtype=np.float64):
    """Marches the rays from x0 along d (n, 3).  dict: fate (0 captured, 1 samples the sky, 2 ran out of iterations), steps,
    esc_dir (the direction after the last step, not normalised), hits: rows (ray, rank, hit_x, hit_y, to_cam xyz), n_hits."""
    t = np.dtype(dtype).type
    n = d.shape[0]
    p = np.broadcast_to(np.asarray(x0, dtype=dtype), (n, 3)).copy()
    dd = np.asarray(d, dtype=dtype).copy()
    tan_t = t(np.tan(np.float32(np.float32(tilt_deg) * np.float32(np.pi) / np.float32(180.0)).astype(dtype)))
    Lv = np.cross(dd, p)
    Ln = np.sqrt(_dot(Lv, Lv))
    m15 = t(-1.5) * (Ln * Ln)
    r_esc, hb = t(np.float32(r_escape)), t(np.float32(h_base))
    max_iter = int(np.float32(r_escape) * np.float32(40.0) / np.float32(h_base))
    max_affine = t(np.float32(r_escape) * np.float32(40.0))
    r2 = _dot(p, p)
    r = np.sqrt(r2)
    f_old = p[:, 2] - p[:, 1] * tan_t
    affine = np.zeros(n, dtype=dtype)
    idx = np.arange(n)
    fate = np.full(n, 2, dtype=np.int8)
    steps = np.zeros(n, dtype=np.int64)
    fin_d = dd.copy()
    n_hits = np.zeros(n, dtype=np.int32)
    hit_rows = []
    half, two, six = t(0.5), t(2), t(6)

    def acc(s, s2, sr):                    # (-1.5 L^2 / r^5) s, r^5 = (r2 r2) r
        return (m15 / (s2 * s2 * sr))[:, None] * s

    it = 0
    while idx.size and it < max_iter:
        h = (hb * K.dt_fac(r))[:, None]
        k1p = h * dd
        k1d = h * acc(p, r2, r)
        s2 = p + half * k1p
        q2 = _dot(s2, s2)
        k2p = h * (dd + half * k1d)
        s3 = p + half * k2p
        q3 = _dot(s3, s3)
        k2d = h * acc(s2, q2, np.sqrt(q2))
        k3p = h * (dd + half * k2d)
        k3d = h * acc(s3, q3, np.sqrt(q3))
        s4 = p + k3p
        q4 = _dot(s4, s4)
        k4p = h * (dd + k3d)
        k4d = h * acc(s4, q4, np.sqrt(q4))
        np_ = p + (((k1p + two * k2p) + two * k3p) + k4p) / six
        nd = dd + (((k1d + two * k2d) + two * k3d) + k4d) / six
        r2n = _dot(np_, np_)
        rn = np.sqrt(r2n)
        aff = affine + h[:, 0]
        captured = rn < t(RS)
        ended = captured | (rn > r_esc) | (aff > max_affine)
        f_new = np_[:, 2] - np_[:, 1] * tan_t
        cross = (f_old * f_new < 0) & ~ended
        if cross.any():
            c = np.nonzero(cross)[0]
            tf = f_old[c] / (f_old[c] - f_new[c] + t(1e-8))
            hx = p[c, 0] + tf * (np_[c, 0] - p[c, 0])
            hy = p[c, 1] + tf * (np_[c, 1] - p[c, 1])
            hr = np.sqrt(hx * hx + hy * hy)
            ok = (t(r_outer) >= hr) & (hr >= t(r_inner))
            c, hx, hy = c[ok], hx[ok], hy[ok]
            if c.size:
                ray = idx[c]
                hit_rows.append(np.column_stack([ray, n_hits[ray], hx, hy, -dd[c, 0], -dd[c, 1], -dd[c, 2]]))
                n_hits[ray] += 1
        it += 1
        steps[idx] = it
        if ended.any():
            e = np.nonzero(ended)[0]
            fate[idx[e]] = np.where(captured[e], 0, 1)
            fin_d[idx[e]] = nd[e]
            keep = ~ended
            idx, p, dd, r, r2, f_old, affine, m15 = idx[keep], np_[keep], nd[keep], rn[keep], r2n[keep], f_new[keep], aff[keep], m15[keep]
        else:
            p, dd, r, r2, f_old, affine = np_, nd, rn, r2n, f_new, aff
    if idx.size:
        fin_d[idx] = dd
    rows = np.concatenate(hit_rows) if hit_rows else np.zeros((0, 7))
    return dict(fate=fate, steps=steps, esc_dir=fin_d, hits=rows, n_hits=n_hits)


# ----------------------------------------------------------------------------------------------- shading
def g_factor(base, hx, hy, hz, hit_r, to_cam, cam_pos, r_inner, r_outer, sin_t, cos_t, D):
    """_apply_g_factor (render.py:2439-2516) for a disk tilted about x, with g = min(g_doppler g_grav D, cap)."""
    t = hx.dtype.type
    rs = t(RS)
    cp = cam_pos.astype(hx.dtype)
    r_obs = np.sqrt((cp[0] * cp[0] + cp[1] * cp[1]) + cp[2] * cp[2])
    r_em = np.sqrt((hx * hx + hy * hy) + hz * hz)
    r_safe = np.maximum(r_em, rs + t(1e-3))
    omega = np.sqrt(t(0.5) / (r_safe * r_safe * r_safe + t(1e-6)))
    lorentz = np.sqrt(np.maximum(t(1) - rs / r_safe, t(1e-6)))
    beta = np.minimum(r_safe * omega / np.maximum(lorentz, t(1e-6)), t(0.99))
    gamma = t(1) / np.sqrt(np.maximum(t(1) - beta * beta, t(1e-6)))
    inv = t(1) / r_em
    rh = np.stack([inv * hx, inv * hy, inv * hz], axis=-1)
    nrm = np.array([t(0), -t(sin_t), t(cos_t)], dtype=hx.dtype)
    vh = np.stack([rh[:, 1] * nrm[2] - rh[:, 2] * nrm[1], rh[:, 2] * nrm[0] - rh[:, 0] * nrm[2], rh[:, 0] * nrm[1] - rh[:, 1] * nrm[0]], axis=-1)
    v_norm = np.sqrt(_dot(vh, vh))
    good = v_norm > t(1e-6)
    vn = np.where(good, v_norm, t(1))[:, None]
    vh = np.where(good[:, None], vh / vn, np.array([t(0), t(1), t(0)], dtype=hx.dtype))
    ti = t(1) / np.sqrt(_dot(to_cam, to_cam))
    cos_theta = _dot(vh, ti[:, None] * to_cam)
    denom = np.maximum(t(1) - beta * cos_theta, t(1e-3))
    g_doppler = t(1) / (gamma * denom)
    grav_num = np.sqrt(np.maximum(t(1) - rs / np.maximum(r_obs, rs + t(1e-3)), t(1e-6)))
    grav_den = np.sqrt(np.maximum(t(1) - rs / np.maximum(r_em, rs + t(1e-3)), t(1e-6)))
    g = np.minimum(g_doppler * (grav_num / grav_den) * D, t(K.G_FACTOR_CAP))
    intensity = np.maximum(g ** t(K.G_LUMINOSITY_POWER), t(0))
    brightness = t(K.G_BRIGHTNESS_GAIN) * intensity / (t(1) + intensity / t(K.G_FACTOR_CAP))
    span = np.maximum(t(r_outer) - t(r_inner), t(1e-3))
    radial_t = np.clip((np.maximum(hit_r, t(r_inner)) - t(r_inner)) / span, t(0), t(1))
    profile = (t(1) - radial_t) ** t(K.DISK_RADIAL_BRIGHTNESS_POWER)
    brightness = brightness * (t(K.DISK_RADIAL_BRIGHTNESS_MIN) + (t(K.DISK_RADIAL_BRIGHTNESS_MAX) - t(K.DISK_RADIAL_BRIGHTNESS_MIN)) * profile)
    wien = t(1) - t(1) / np.maximum(g, t(0.1))
    r_s_, g_s_, b_s_ = np.exp(t(2.21) * wien), np.exp(t(2.72) * wien), np.exp(t(3.13) * wien)
    r_s_ = np.minimum(r_s_ / g_s_, t(3))
    b_s_ = np.minimum(b_s_ / g_s_, t(3))
    tint = K.disk_tint(t)
    out = np.stack([base[:, 0] * r_s_ * tint[0] * brightness, base[:, 1] * tint[1] * brightness,
                    base[:, 2] * b_s_ * tint[2] * brightness], axis=-1)
    return np.clip(out, t(0), t(10))


def render(cam, beta, sky, tex, h_base=0.1, r_inner=2.0, r_outer=15.0, tilt_deg=0.0, t_offset=0.0, sky_shift_on=True, dtype=np.float64):
    """One frame of the camera `cam` (kerr_ref.build_camera) moving with beta: dict with bg, disk as (H, W, 3) in `dtype`,
    fate, n_hits, steps as (H, W), D (H, W) and n (H, W, 3)."""
    t = np.dtype(dtype).type
    W, H = cam["width"], cam["height"]
    npr = K.pixel_rays(cam, dtype).reshape(-1, 3)
    n_dir, D = aberrate(npr, beta, dtype)
    m = march(cam["pos"].astype(dtype), n_dir, h_base, cam["r_escape"], r_inner, r_outer, tilt_deg, dtype)
    tilt = np.float32(np.float32(tilt_deg) * np.float32(np.pi) / np.float32(180.0)).astype(dtype)
    tan_t, sin_t, cos_t = t(np.tan(tilt)), t(np.sin(tilt)), t(np.cos(tilt))
    n = W * H
    accum = np.zeros((n, 3), dtype=dtype)
    alpha = np.zeros(n, dtype=dtype)
    rows = m["hits"]
    for k in range(int(rows[:, 1].max()) + 1 if rows.shape[0] else 0):       # front to back
        sel = rows[rows[:, 1] == k]
        ray = sel[:, 0].astype(np.int64)
        hx, hy, to_cam = sel[:, 2].astype(dtype), sel[:, 3].astype(dtype), sel[:, 4:7].astype(dtype)
        hit_r = np.sqrt(hx * hx + hy * hy)
        rgba = K.sample_disk(tex, hx, hy, hit_r, 0.0, r_inner, r_outer, t_offset)
        base_alpha = np.minimum(rgba[:, 3], t(0.999))
        disk_alpha = t(1) - (t(1) - base_alpha) ** t(K.DISK_ALPHA_GAIN)
        col = g_factor(rgba[:, :3], hx, hy, hy * tan_t, hit_r, to_cam, cam["pos"], r_inner, r_outer, sin_t, cos_t, D[ray])
        front = t(1) - alpha[ray]
        accum[ray] = accum[ray] + col * disk_alpha[:, None] * front[:, None]
        alpha[ray] = t(1) - front * (t(1) - disk_alpha)
    bg = np.zeros((n, 3), dtype=dtype)
    esc = m["fate"] == 1
    if esc.any():
        e = m["esc_dir"][esc].astype(dtype)
        e = (t(1) / np.sqrt(_dot(e, e)))[:, None] * e
        c = K.sample_skybox(sky, e)
        if sky_shift_on:
            c = sky_shift(c, D[esc])
        bg[esc] = c * (t(1) - alpha[esc])[:, None]
    disk = np.clip(accum, t(0), t(1))
    sh = (H, W)
    return dict(bg=bg.reshape(H, W, 3), disk=disk.reshape(H, W, 3), fate=m["fate"].reshape(sh), n_hits=m["n_hits"].reshape(sh),
                steps=m["steps"].reshape(sh), D=D.reshape(sh), n=n_dir.reshape(H, W, 3))
