"""CPU reference of the exact disk redshift of the spinning (Kerr) hole (`--redshift exact`; DESIGN.md "Kerr"), in NumPy.

The march is kerr_ref's (rk4_step, dt_fac, initial_momentum, ks_radius), the sampler and everything behind the g-factor
are kerr_ref's; what is new is the photon's momentum at a disk crossing and the g-factor made from it.  Units r_s = 1,
M = 1/2, a = A M signed.  The traced ray is the future-directed photon with p_t = -1; the disk turns in the +phi sense
with Omega > 0 around a hole of the signed a.  Frequencies are -p.u at the two ends of the ray, g = nu_obs / nu_em:

    observer   static at the camera: nu_obs = 1 / sqrt(1 - f_cam), f_cam = r / S there
    photon     at the hit (hx, hy, 0), momentum interpolated like the hit point, p_hit = p + t_frac (np - p):
               L_z = hx p_y - hy p_x,   P = (hx p_x + hy p_y) / rho,   U = 1 + l.p_hit = 1 + (r P - a L_z / rho) / rho
               with rho^2 = hx^2 + hy^2 = r^2 + a^2
    emitter    r >= r_isco: the circular geodesic, nu_em = (1 - Omega L_z) / sqrt(1 - Omega^2 rho^2 - (1 - a Omega)^2 / r)
               r <  r_isco: the ISCO's E and L kept, falling inward (nu_em_plunge)

Everything is vectorised and runs in `dtype`.  Nothing here imports the product package.
"""
import numpy as np

import kerr_ref as K

M = K.M
NU_EM_MIN = 1e-3
RADICAND_MIN = 1e-6


# ----------------------------------------------------------------------------------------------- the ISCO orbit
def bardeen_energy_momentum(r, a):
    """E = -u_t and L = u_phi of the circular equatorial geodesic at r that turns in the +phi sense (Bardeen, Press,
    Teukolsky 1972), signed a."""
    sm = np.sqrt(M)
    den = r ** 0.75 * np.sqrt(r ** 1.5 - 3.0 * M * np.sqrt(r) + 2.0 * a * sm)
    E = (r ** 1.5 - 2.0 * M * np.sqrt(r) + a * sm) / den
    L = sm * (r * r - 2.0 * a * sm * np.sqrt(r) + a * a) / den
    return E, L


def isco_orbit(A):
    """(r_isco, E, L) of the disk's sense of rotation in binary64: prograde for A >= 0, retrograde for A < 0."""
    A = float(A)
    r = float(K.r_isco(A, A >= 0))
    E, L = bardeen_energy_momentum(r, A * M)
    return r, float(E), float(L)


def omega_exact(r, a):
    """Kerr's orbital frequency without the reference's 1e-6 guard (omega_kerr has it)."""
    sm = np.sqrt(r.dtype.type(M))
    return sm / (r * np.sqrt(r) + r.dtype.type(a) * sm)


# ----------------------------------------------------------------------------------------------- frequencies
def nu_observer(cam_pos, a, dtype):
    t = np.dtype(dtype).type
    x = np.asarray(cam_pos).astype(dtype)
    a2 = t(a) * t(a)
    w = (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) - a2
    S = np.sqrt(w * w + t(4) * a2 * (x[2] * x[2]))
    r = np.sqrt(t(0.5) * (w + S))
    return t(1) / np.sqrt(t(1) - r / S)


def circular_radicand(r, a, omega):
    """1 / (u^t)^2 of the circular orbit of frequency omega at r."""
    t = r.dtype.type
    a = t(a)
    q = t(1) - a * omega
    return t(1) - omega * omega * (r * r + a * a) - q * q / r


def nu_em_circular(r, a, lz, omega):
    t = r.dtype.type
    return (t(1) - omega * lz) / np.sqrt(np.maximum(circular_radicand(r, a, omega), t(RADICAND_MIN)))


def plunge_discriminant(r, a, r_isco, E, L):
    """qb^2 - 4 qa qc of plunge_velocity's quadratic, literally: what the closed form below is checked against."""
    t = r.dtype.type
    a, E, L = t(a), t(E), t(L)
    rho2 = r * r + a * a
    c0 = E - a * L / rho2
    qa = t(1) - r / rho2
    qb = t(-2) * c0 / np.sqrt(rho2)
    qc = t(1) - E * E + L * L / rho2 - c0 * c0 / r
    return qb * qb - t(4) * qa * qc


def plunge_velocity(r, a, r_isco, E, L):
    """(w, S) of the gas that fell from the ISCO with its E and L: the covariant velocity is u_t = -E with the spatial part
    (L / rho) e_phi + w e_rho, S = l^mu u_mu; w is the inward root of g^{mu nu} u_mu u_nu = -1, the quadratic
    qa w^2 + qb w + qc = 0.  Its discriminant is 4 (u^rho)^2, and with the ISCO's E and L the radial potential has its triple
    root at r_isco: qb^2 - 4 qa qc = 4 (1 - E^2) (r_isco - r)^3 / (r rho^2).  That form is what is evaluated: the literal
    one is a difference of two numbers of order one that vanishes at r_isco, and its square root there is the square root
    of the rounding (1e-8 in binary64, 3e-4 in binary32)."""
    t = r.dtype.type
    a, E, L = t(a), t(E), t(L)
    rho2 = r * r + a * a
    rho = np.sqrt(rho2)
    c0 = E - a * L / rho2
    qa = t(1) - r / rho2
    qb = t(-2) * c0 / rho
    dr = np.maximum(t(r_isco) - r, t(0))
    disc = t(4) * ((t(1) - E) * (t(1) + E)) * (dr * dr * dr) / (r * rho2)
    w = (-qb - np.sqrt(disc)) / (t(2) * qa)
    return w, c0 + r * w / rho


def nu_em_plunge(r, a, lz, P, U, r_isco, E, L):
    t = r.dtype.type
    w, S = plunge_velocity(r, a, r_isco, E, L)
    return t(E) - t(L) * lz / (r * r + t(a) * t(a)) - w * P + U * S / r


def g_exact(hx, hy, lz, P, U, a, cam_pos, isco):
    """The g-factor of a crossing at (hx, hy) whose photon has (L_z, P, U) there; isco = (r_isco, E, L)."""
    t = hx.dtype.type
    r_isco, E, L = isco
    r = np.sqrt(hx * hx + hy * hy - t(a) * t(a))
    nu_c = nu_em_circular(r, a, lz, K.omega_kerr(r, a))
    with np.errstate(invalid="ignore", divide="ignore"):
        nu_p = nu_em_plunge(r, a, lz, P, U, r_isco, E, L)
    nu_em = np.where(r >= t(r_isco), nu_c, nu_p)
    return np.minimum(nu_observer(cam_pos, a, hx.dtype) / np.maximum(nu_em, t(NU_EM_MIN)), t(K.G_FACTOR_CAP))


def shade_g(base, g, hit_r, r_inner, r_outer):
    """kerr_ref.g_factor from its g on: intensity power, brightness, radial profile, Wien tint, clamp at 10."""
    t = g.dtype.type
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


# ----------------------------------------------------------------------------------------------- the march
def march(x0, d, A, h_base=0.1, r_escape=12.0, r_inner=2.0, r_outer=15.0, dtype=np.float64):
    """kerr_ref.march with the photon at each crossing: the rows of `hits` are (ray, rank, hx, hy, L_z, P, U)."""
    t = np.dtype(dtype).type
    a = t(A) * t(M)
    n = d.shape[0]
    x = np.broadcast_to(np.asarray(x0, dtype=dtype), (n, 3)).copy()
    p = K.initial_momentum(x, np.asarray(d, dtype=dtype), a)
    rp = t(K.r_plus(float(A)))
    r_esc, hb = t(r_escape), t(h_base)
    max_iter = int(np.float32(r_escape) * np.float32(40.0) / np.float32(h_base))
    max_affine = t(np.float32(r_escape) * np.float32(40.0))
    r = K.ks_radius(x, a)
    affine = np.zeros(n, dtype=dtype)
    idx = np.arange(n)
    fate = np.full(n, 2, dtype=np.int8)
    steps = np.zeros(n, dtype=np.int64)
    fin_x, fin_p = x.copy(), p.copy()
    n_hits = np.zeros(n, dtype=np.int32)
    hit_rows = []
    it = 0
    while idx.size and it < max_iter:
        h = hb * K.dt_fac(r)
        nx, npm, _ = K.rk4_step(x, p, h, a)
        rn = K.ks_radius(nx, a)
        aff = affine + h
        captured = rn < rp
        ended = captured | (rn > r_esc) | (aff > max_affine)
        z0, z1 = x[:, 2], nx[:, 2]
        cross = (z0 * z1 < 0) & ~ended
        if cross.any():
            c = np.nonzero(cross)[0]
            tf = z0[c] / (z0[c] - z1[c] + t(1e-8))
            hx = x[c, 0] + tf * (nx[c, 0] - x[c, 0])
            hy = x[c, 1] + tf * (nx[c, 1] - x[c, 1])
            rho2 = hx * hx + hy * hy
            hr = np.sqrt(rho2 - a * a)
            ok = (t(r_outer) >= hr) & (hr >= t(r_inner))
            c, tf, hx, hy, rho2, hr = c[ok], tf[ok], hx[ok], hy[ok], rho2[ok], hr[ok]
            if c.size:
                px = p[c, 0] + tf * (npm[c, 0] - p[c, 0])
                py = p[c, 1] + tf * (npm[c, 1] - p[c, 1])
                irho = t(1) / np.sqrt(rho2)
                lz = hx * py - hy * px
                P = (hx * px + hy * py) * irho
                U = t(1) + (hr * P - a * lz * irho) * irho
                ray = idx[c]
                hit_rows.append(np.column_stack([ray, n_hits[ray], hx, hy, lz, P, U]))
                n_hits[ray] += 1
        it += 1
        steps[idx] = it
        if ended.any():
            e = np.nonzero(ended)[0]
            fate[idx[e]] = np.where(captured[e], 0, 1)
            fin_x[idx[e]], fin_p[idx[e]] = nx[e], npm[e]
            keep = ~ended
            idx, x, p, r, affine = idx[keep], nx[keep], npm[keep], rn[keep], aff[keep]
        else:
            x, p, r, affine = nx, npm, rn, aff
    if idx.size:
        fin_x[idx], fin_p[idx] = x, p
    v, _ = K.rhs(fin_x, fin_p, a)
    esc = v / np.sqrt((v * v).sum(-1))[:, None]
    rows = np.concatenate(hit_rows) if hit_rows else np.zeros((0, 7))
    return dict(fate=fate, steps=steps, esc_dir=esc, hits=rows, n_hits=n_hits, x=fin_x, p=fin_p)


def render(cam, A, sky, tex, h_base=0.1, r_inner=2.0, r_outer=15.0, t_offset=0.0, dtype=np.float64):
    """kerr_ref.render's frame dict under the exact redshift, and first_g (H, W): the g-factor of a ray's first crossing
    (NaN without one)."""
    t = np.dtype(dtype).type
    K.check_camera(cam["pos"], A)
    W, H = cam["width"], cam["height"]
    d = K.pixel_rays(cam, dtype).reshape(-1, 3)
    m = march(cam["pos"].astype(dtype), d, A, h_base, cam["r_escape"], r_inner, r_outer, dtype)
    a = t(A) * t(M)
    isco = isco_orbit(A)
    n = W * H
    accum = np.zeros((n, 3), dtype=dtype)
    alpha = np.zeros(n, dtype=dtype)
    rows = m["hits"]
    first = np.full((n, 2), np.nan)
    first_g = np.full(n, np.nan)
    for k in range(int(rows[:, 1].max()) + 1 if rows.shape[0] else 0):       # front to back
        sel = rows[rows[:, 1] == k]
        ray = sel[:, 0].astype(np.int64)
        hx, hy, lz, P, U = (sel[:, c].astype(dtype) for c in range(2, 7))
        hit_r = np.sqrt(hx * hx + hy * hy - a * a)
        g = g_exact(hx, hy, lz, P, U, a, cam["pos"], isco)
        if k == 0:
            first[ray] = sel[:, 2:4]
            first_g[ray] = g
        rgba = K.sample_disk(tex, hx, hy, hit_r, a, r_inner, r_outer, t_offset)
        base_alpha = np.minimum(rgba[:, 3], t(0.999))
        disk_alpha = t(1) - (t(1) - base_alpha) ** t(K.DISK_ALPHA_GAIN)
        col = shade_g(rgba[:, :3], g, hit_r, r_inner, r_outer)
        front = t(1) - alpha[ray]
        accum[ray] = accum[ray] + col * (disk_alpha * front)[:, None]
        alpha[ray] = t(1) - front * (t(1) - disk_alpha)
    bg = np.zeros((n, 3), dtype=dtype)
    esc = m["fate"] == 1
    if esc.any():
        bg[esc] = K.sample_skybox(sky, m["esc_dir"][esc].astype(dtype)) * (t(1) - alpha[esc])[:, None]
    disk = np.clip(accum, t(0), t(1))
    sh = (H, W)
    return dict(bg=bg.reshape(H, W, 3), disk=disk.reshape(H, W, 3), final=np.clip(bg + disk, t(0), t(1)).reshape(H, W, 3),
                fate=m["fate"].reshape(sh), n_hits=m["n_hits"].reshape(sh), steps=m["steps"].reshape(sh),
                esc_dir=np.where(esc[:, None], m["esc_dir"], 0.0).reshape(H, W, 3), first_hit=first.reshape(H, W, 2),
                first_g=first_g.reshape(sh))
