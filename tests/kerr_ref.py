"""CPU reference of the spinning (Kerr) hole: the model of DESIGN.md "Kerr", statement by statement, in NumPy.

Units as everywhere in this project: r_s = 1, M = 1/2.  The spin is A = a / M with |A| <= 0.998, a = A M.  Kerr-Schild
Cartesian coordinates, the spin axis is z:

    r^2 = ((rho2 - a^2) + sqrt((rho2 - a^2)^2 + 4 a^2 z^2)) / 2,   rho2 = x.x
    f   = r_s r^3 / (r^4 + a^2 z^2)
    l   = ((r x + a y) / (r^2 + a^2), (r y - a x) / (r^2 + a^2), z / r)
    H   = (p.p - 1) / 2 - f (1 + l.p)^2 / 2                        (p_t = -1)
    dx/dl = p - f (1 + l.p) l,   dp/dl = -grad_x H

`hamiltonian` evaluates these formulas literally.  `rhs` is what the march integrates -- the same quantities written the
way the device kernel (csrc/ray_kerr.h) writes them: with S = sqrt((rho2 - a^2)^2 + 4 a^2 z^2) = 2 r^2 - (rho2 - a^2) one
has r^4 + a^2 z^2 = r^2 S, hence f = r / S, and

    grad r = (r^2 x + a^2 z e_z) / (r S)
    grad S = (2 (rho2 - a^2) x + 4 a^2 z e_z) / S
    grad f = (grad r - f grad S) / S
    grad (l.p) = ((r p_x - a p_y) / Q, (a p_x + r p_y) / Q, p_z / r) + d(l.p)/dr grad r,        Q = r^2 + a^2
    d(l.p)/dr  = (x p_x + y p_y) / Q - 2 r N / Q^2 - z p_z / r^2,   N = r (x p_x + y p_y) + a (y p_x - x p_y)
    dp/dl = (u^2 / 2) grad f + f u grad (l.p),                       u = 1 + l.p

tests/test_kerr_ref.py checks them against central differences of `hamiltonian`.

Everything is vectorised over rays and runs in `dtype` (float64 by default, float32 to measure what the number format
costs).  Nothing here imports the product package.
"""
import numpy as np

M = 0.5
RS = 1.0
A_MAX = 0.998
G_FACTOR_CAP = 1.5
G_LUMINOSITY_POWER = 1.5
G_BRIGHTNESS_GAIN = 0.38
DISK_COLOR_TEMPERATURE = 6000.0
DISK_ALPHA_GAIN = 6.0
DISK_RADIAL_BRIGHTNESS_POWER = 1.2
DISK_RADIAL_BRIGHTNESS_MIN = 0.2
DISK_RADIAL_BRIGHTNESS_MAX = 8.0


# ----------------------------------------------------------------------------------------------- radii of the metric
def r_plus(A):
    return (1.0 + np.sqrt(1.0 - A * A)) / 2.0


def r_isco(A, prograde=True):
    """Bardeen's formula, in r_s = 1 units; prograde: the orbit turns with the hole."""
    A = abs(float(A))
    z1 = 1.0 + (1.0 - A * A) ** (1.0 / 3.0) * ((1.0 + A) ** (1.0 / 3.0) + (1.0 - A) ** (1.0 / 3.0))
    z2 = np.sqrt(3.0 * A * A + z1 * z1)
    s = -1.0 if prograde else 1.0
    return M * (3.0 + z2 + s * np.sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2)))


def r_photon(A, prograde=True):
    A = abs(float(A))
    return 2.0 * M * (1.0 + np.cos(2.0 / 3.0 * np.arccos(-A if prograde else A)))


def shadow_edges(A):
    """(b_pro, b_retro): L_z / E of the two equatorial critical photons, b = +-3 sqrt(M r_ph) - a, for the hole of spin A
    in the march's chart (positive A: photons with L_z > 0 are the prograde ones)."""
    a = abs(A) * M
    bp = 3.0 * np.sqrt(M * r_photon(A, True)) - a
    br = -3.0 * np.sqrt(M * r_photon(A, False)) - a
    return (bp, br) if A >= 0 else (-br, -bp)


def kerr_info(A):
    return dict(a=A * M, r_plus=r_plus(A), r_isco_prograde=r_isco(A, True), r_isco_retrograde=r_isco(A, False),
                r_photon_pro=r_photon(A, True), r_photon_retro=r_photon(A, False))


# ----------------------------------------------------------------------------------------------- geometry
def ks_radius(x, a):
    t = x.dtype.type
    a2 = t(a) * t(a)
    w = (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1] + x[..., 2] * x[..., 2]) - a2
    S = np.sqrt(w * w + t(4) * a2 * (x[..., 2] * x[..., 2]))
    return np.sqrt(t(0.5) * (w + S))


def geometry(x, a):
    """r, f, l of the formulas in the module docstring, literally."""
    t = x.dtype.type
    a = t(a)
    r = ks_radius(x, a)
    z = x[..., 2]
    f = t(RS) * r ** 3 / (r ** 4 + a * a * z * z)
    q = r * r + a * a
    l = np.stack([(r * x[..., 0] + a * x[..., 1]) / q, (r * x[..., 1] - a * x[..., 0]) / q, z / r], axis=-1)
    return r, f, l


def hamiltonian(x, p, a):
    t = x.dtype.type
    _, f, l = geometry(x, a)
    u = t(1) + (l * p).sum(-1)
    return t(0.5) * ((p * p).sum(-1) - t(1)) - t(0.5) * f * u * u


def l_z(x, p):
    return x[..., 0] * p[..., 1] - x[..., 1] * p[..., 0]


def rhs(x, p, a):
    """(dx/dl, dp/dl) in the kernel's own form (module docstring)."""
    t = x.dtype.type
    a = t(a)
    a2 = a * a
    X, Y, Z = x[..., 0], x[..., 1], x[..., 2]
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    w = (X * X + Y * Y + Z * Z) - a2
    S = np.sqrt(w * w + t(4) * a2 * (Z * Z))
    r2 = t(0.5) * (w + S)
    r = np.sqrt(r2)
    iS, ir, iQ = t(1) / S, t(1) / r, t(1) / (r2 + a2)
    f = r * iS
    lx, ly, lz = (r * X + a * Y) * iQ, (r * Y - a * X) * iQ, Z * ir
    u = t(1) + (lx * px + ly * py + lz * pz)
    fu = f * u
    v = np.stack([px - fu * lx, py - fu * ly, pz - fu * lz], axis=-1)
    g = ir * iS
    grx, gry, grz = r2 * X * g, r2 * Y * g, (r2 + a2) * Z * g
    w2 = t(2) * w
    gfx = (grx - f * (w2 * X * iS)) * iS
    gfy = (gry - f * (w2 * Y * iS)) * iS
    gfz = (grz - f * ((w2 + t(4) * a2) * Z * iS)) * iS
    sxy = X * px + Y * py
    N = r * sxy + a * (Y * px - X * py)
    dr = sxy * iQ - t(2) * r * N * iQ * iQ - Z * pz * ir * ir
    glx = (r * px - a * py) * iQ + dr * grx
    gly = (a * px + r * py) * iQ + dr * gry
    glz = pz * ir + dr * grz
    c1 = t(0.5) * u * u
    dp = np.stack([c1 * gfx + fu * glx, c1 * gfy + fu * gly, c1 * gfz + fu * glz], axis=-1)
    return v, dp


def initial_momentum(x, d, a):
    """The momentum of the future-directed photon whose coordinate velocity at x is parallel to the unit vector d."""
    t = x.dtype.type
    _, f, l = geometry(x, a)
    c = (l * d).sum(-1)
    s = t(1) / np.sqrt(t(1) - f * (t(1) - c * c))
    lam = (t(1) + s * c) / (t(1) - f)
    return s[..., None] * d + (f * lam)[..., None] * l


def camera_f(cam_pos, A):
    """(f, r) of a camera position in binary64: f = r / S and the Kerr-Schild radius r."""
    x = np.asarray(cam_pos).astype(np.float64)
    a2 = (float(A) * M) ** 2
    w = float((x * x).sum()) - a2
    S = float(np.sqrt(w * w + 4.0 * a2 * float(x[2]) ** 2))
    r = float(np.sqrt(0.5 * (w + S)))
    return (r / S if S > 0 else np.inf), r


def check_camera(cam_pos, A):
    """The domain of the camera (include/bhr.h: bhr_set_spin): outside the static limit f = 1, where initial_momentum's
    s = 1 / sqrt(1 - f (1 - c^2)) is real for every direction and a static observer exists, and outside the horizon.  The
    library refuses a render from anywhere else before it launches, and so does this reference."""
    f, r = camera_f(cam_pos, A)
    if not (f < 1.0 and r >= r_plus(float(A))):
        raise ValueError(f"camera at {tuple(float(v) for v in cam_pos)} lies inside the static limit of the hole of spin {A:g} "
                         f"(f = r / S = {f:g} >= 1 or r = {r:g} inside the horizon at {r_plus(float(A)):g})")


def dt_fac(r):
    """The reference's step factor (render.py:2865-2868) on the Kerr-Schild radius: r_cap = r_s = 1, max_fac 10."""
    t = r.dtype.type
    r_safe = np.maximum(r, t(RS) + t(1e-3))
    far = np.minimum(np.sqrt(r_safe), t(10))
    q = t(1) / r_safe
    near = t(1) / (t(1) + t(2) * (q * q * q))
    return np.clip(far * near, t(0.2), t(10))


def rk4_step(x, p, h, a):
    """One RK4 step of size h (per ray) on (x, p); also dx/dl at the start of the step."""
    t = x.dtype.type
    hh = h[..., None]
    v1, a1 = rhs(x, p, a)
    v2, a2_ = rhs(x + t(0.5) * hh * v1, p + t(0.5) * hh * a1, a)
    v3, a3 = rhs(x + t(0.5) * hh * v2, p + t(0.5) * hh * a2_, a)
    v4, a4 = rhs(x + hh * v3, p + hh * a3, a)
    six = t(1) / t(6)
    nx = x + hh * ((v1 + t(2) * v2 + t(2) * v3 + v4) * six)
    npm = p + hh * ((a1 + t(2) * a2_ + t(2) * a3 + a4) * six)
    return nx, npm, v1


# ----------------------------------------------------------------------------------------------- camera
def build_camera(cam_pos, fov_deg, width, height, r_max=10.0):
    """The f32 camera uniforms a frame is rendered from (f64 pin-hole camera looking at the origin, cast to f32)."""
    p = np.array(cam_pos, dtype=np.float64)
    fwd = -p / np.linalg.norm(p)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    rn = np.linalg.norm(right)
    right = np.array([1.0, 0.0, 0.0]) if rn < 1e-6 else right / rn
    up = np.cross(right, fwd)
    up /= np.linalg.norm(up)
    plane_h = 2.0 * np.tan(np.radians(fov_deg) / 2)
    plane_w = plane_h * (width / height)
    f32 = np.float32
    return dict(pos=p.astype(f32), right=right.astype(f32), up=up.astype(f32), forward=fwd.astype(f32),
                pw=f32(plane_w / width), ph=f32(plane_h / height), r_escape=f32(max(r_max, float(np.linalg.norm(p)) * 2)),
                width=int(width), height=int(height))


def pixel_rays(cam, dtype=np.float64):
    """Unit pixel directions (H, W, 3) of the camera (render.py:2811-2840)."""
    t = np.dtype(dtype).type
    W, H = cam["width"], cam["height"]
    cp, cr, cu, cf = (cam[k].astype(dtype) for k in ("pos", "right", "up", "forward"))
    pw, ph = t(cam["pw"]), t(cam["ph"])
    center = cp + cf
    half_w, half_h = pw * t(W) / t(2), ph * t(H) / t(2)
    tl = (center - half_w * cr) + half_h * cu
    i = np.arange(W, dtype=dtype)[None, :, None]
    j = np.arange(H, dtype=dtype)[:, None, None]
    pos = (tl + ((i + t(0.5)) * pw) * cr) - ((j + t(0.5)) * ph) * cu
    d = pos - cp
    inv = t(1) / np.sqrt((d * d).sum(-1))
    return (inv[..., None] * d).astype(dtype)


# ----------------------------------------------------------------------------------------------- the march
def march(x0, d, A, h_base=0.1, r_escape=12.0, r_inner=2.0, r_outer=15.0, dtype=np.float64, want_path=False, path_r_min=0.0):
    """Marches the rays (n, 3) from x0 along the unit directions d.  Returns a dict:
    fate (0 captured, 1 escaped: samples the sky, 2 ran out of iterations), steps, esc_dir (direction of dx/dl at the last
    state), hits: a list, per crossing rank k, of (ray index array, hit_x, hit_y, to_cam (m, 3)); n_hits per ray; with
    want_path also dH, dL: the largest |H - H0| and |L_z - L_z0| over each ray's states outside the horizon with r >= path_r_min."""
    t = np.dtype(dtype).type
    a = t(A) * t(M)
    n = d.shape[0]
    x = np.broadcast_to(np.asarray(x0, dtype=dtype), (n, 3)).copy()
    dd = np.asarray(d, dtype=dtype)
    p = initial_momentum(x, dd, a)
    rp = t(r_plus(float(A)))
    r_esc, hb = t(r_escape), t(h_base)
    max_iter = int(np.float32(r_escape) * np.float32(40.0) / np.float32(h_base))
    max_affine = t(np.float32(r_escape) * np.float32(40.0))
    r = ks_radius(x, a)
    affine = np.zeros(n, dtype=dtype)
    idx = np.arange(n)
    fate = np.full(n, 2, dtype=np.int8)
    steps = np.zeros(n, dtype=np.int64)
    fin_x, fin_p = x.copy(), p.copy()
    n_hits = np.zeros(n, dtype=np.int32)
    hit_rows = []                      # (ray, rank, hx, hy, tcx, tcy, tcz)
    if want_path:
        H0, L0 = hamiltonian(x, p, a), l_z(x, p)
        dH, dL = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    it = 0
    while idx.size and it < max_iter:
        h = hb * dt_fac(r)
        nx, npm, v1 = rk4_step(x, p, h, a)
        rn = ks_radius(nx, a)
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
            hr = np.sqrt(hx * hx + hy * hy - a * a)
            ok = (t(r_outer) >= hr) & (hr >= t(r_inner))
            c, hx, hy = c[ok], hx[ok], hy[ok]
            if c.size:
                ray = idx[c]
                hit_rows.append(np.column_stack([ray, n_hits[ray], hx, hy, -v1[c, 0], -v1[c, 1], -v1[c, 2]]))
                n_hits[ray] += 1
        it += 1
        steps[idx] = it
        if want_path:
            on = ~captured & (rn >= t(path_r_min))   # a captured ray ends at the horizon: the state behind it is not part of the ray
            dH[idx[on]] = np.maximum(dH[idx[on]], np.abs(hamiltonian(nx[on], npm[on], a) - H0[idx[on]]))
            dL[idx[on]] = np.maximum(dL[idx[on]], np.abs(l_z(nx[on], npm[on]) - L0[idx[on]]))
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
    v, _ = rhs(fin_x, fin_p, a)
    esc = v / np.sqrt((v * v).sum(-1))[:, None]
    rows = np.concatenate(hit_rows) if hit_rows else np.zeros((0, 7))
    out = dict(fate=fate, steps=steps, esc_dir=esc, hits=rows, n_hits=n_hits, x=fin_x, p=fin_p)
    if want_path:
        out["dH"], out["dL"] = dH, dL
    return out


# ----------------------------------------------------------------------------------------------- shading
def _pymod(a, m):
    return np.mod(a, m)


def sample_skybox(sky, d):
    """_sample_skybox (render.py:2541-2566); d (n, 3) unit."""
    t = d.dtype.type
    tex_h, tex_w = sky.shape[:2]
    sky = sky.astype(d.dtype)
    two_pi, pi = t(np.float32(2 * np.pi)), t(np.float32(np.pi))
    theta = np.arccos(np.clip(d[:, 2], t(-1), t(1)))
    phi = np.arctan2(d[:, 1], d[:, 0])
    phi = np.where(phi < 0, phi + two_pi, phi)
    u = phi / two_pi * t(tex_w)
    v = theta / pi * t(tex_h)
    u0, v0 = np.floor(u), np.floor(v)
    fu, fv = (u - u0)[:, None], (v - v0)[:, None]
    u0, v0 = u0.astype(np.int64), v0.astype(np.int64)
    u0w, u1w = _pymod(u0, tex_w), _pymod(u0 + 1, tex_w)
    v0h, v1h = np.clip(v0, 0, tex_h - 1), np.clip(v0 + 1, 0, tex_h - 1)
    one = t(1)
    return (sky[v0h, u0w] * (one - fu) * (one - fv) + sky[v0h, u1w] * fu * (one - fv) + sky[v1h, u0w] * (one - fu) * fv
            + sky[v1h, u1w] * fu * fv)


def omega_kerr(r, a):
    """sqrt(M) / (r^1.5 + a sqrt(M)) with the reference's guards: sqrt(0.5 / (r^3 + 1e-6)) at a = 0."""
    t = r.dtype.type
    sm = np.sqrt(t(0.5))
    return sm / (np.sqrt(r * r * r + t(1e-6)) + t(a) * sm)


def sample_disk(tex, hx, hy, hit_r, a, r_inner, r_outer, t_offset):
    """_sample_disk (render.py:2568-2600) with the Boyer-Lindquist hit radius and Kerr's Omega in the roll."""
    t = hx.dtype.type
    n_r, n_phi = tex.shape[:2]
    tex = tex.astype(hx.dtype)
    two_pi = t(np.float32(2 * np.pi))
    phi = np.arctan2(hy, hx)
    r_safe = np.maximum(hit_r, t(1e-3))
    phi = phi + t(t_offset) * omega_kerr(r_safe, a)
    phi = np.mod(phi, two_pi)
    phi = np.where(phi >= two_pi, phi - two_pi, phi)
    u = phi / two_pi * t(n_phi)
    v = (hit_r - t(r_inner)) / (t(r_outer) - t(r_inner)) * t(n_r)
    u0, v0 = np.floor(u), np.floor(v)
    fu, fv = (u - u0)[:, None], (v - v0)[:, None]
    u0, v0 = u0.astype(np.int64), v0.astype(np.int64)
    u0w, u1w = _pymod(u0, n_phi), _pymod(u0 + 1, n_phi)
    v0h, v1h = np.clip(v0, 0, n_r - 1), np.clip(v0 + 1, 0, n_r - 1)
    one = t(1)
    return (tex[v0h, u0w] * (one - fu) * (one - fv) + tex[v0h, u1w] * fu * (one - fv) + tex[v1h, u0w] * (one - fu) * fv
            + tex[v1h, u1w] * fu * fv)


def disk_tint(t):
    T = t(DISK_COLOR_TEMPERATURE) / t(100)
    g = np.clip(t(0.390082) * np.log(np.maximum(T, t(0.0001))) - t(0.631841), t(0), t(1))
    b = np.clip(t(0.543207) * np.log(np.maximum(T - t(10), t(0.0001))) - t(1.19625), t(0), t(1))
    return np.array([t(1), g, b], dtype=t)


def g_factor(base, hx, hy, hit_r, to_cam, a, cam_pos, r_inner, r_outer):
    """_apply_g_factor (render.py:2439-2516) for the untilted disk; the emitter's radius is the Boyer-Lindquist hit radius
    and the orbital frequency Kerr's."""
    t = hx.dtype.type
    rs = t(RS)
    r_obs = np.sqrt((cam_pos.astype(hx.dtype) ** 2).sum())
    r_em = hit_r
    r_safe = np.maximum(r_em, rs + t(1e-3))
    omega = omega_kerr(r_safe, a)
    lorentz = np.sqrt(np.maximum(t(1) - rs / r_safe, t(1e-6)))
    beta = np.minimum(r_safe * omega / np.maximum(lorentz, t(1e-6)), t(0.99))
    gamma = t(1) / np.sqrt(np.maximum(t(1) - beta * beta, t(1e-6)))
    inv = t(1) / np.sqrt(hx * hx + hy * hy)
    rx, ry = inv * hx, inv * hy
    vx, vy = ry, -rx                                  # r_hat x n, n = (0, 0, 1)
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
    g = np.minimum(g_doppler * (grav_num / grav_den), t(G_FACTOR_CAP))
    intensity = np.maximum(g ** t(G_LUMINOSITY_POWER), t(0))
    brightness = t(G_BRIGHTNESS_GAIN) * intensity / (t(1) + intensity / t(G_FACTOR_CAP))
    span = np.maximum(t(r_outer) - t(r_inner), t(1e-3))
    radial_t = np.clip((np.maximum(hit_r, t(r_inner)) - t(r_inner)) / span, t(0), t(1))
    profile = (t(1) - radial_t) ** t(DISK_RADIAL_BRIGHTNESS_POWER)
    brightness = brightness * (t(DISK_RADIAL_BRIGHTNESS_MIN) + (t(DISK_RADIAL_BRIGHTNESS_MAX) - t(DISK_RADIAL_BRIGHTNESS_MIN)) * profile)
    wien = t(1) - t(1) / np.maximum(g, t(0.1))
    r_s_, g_s_, b_s_ = np.exp(t(2.21) * wien), np.exp(t(2.72) * wien), np.exp(t(3.13) * wien)
    r_s_ = np.minimum(r_s_ / g_s_, t(3))
    b_s_ = np.minimum(b_s_ / g_s_, t(3))
    tint = disk_tint(t)
    out = np.stack([base[:, 0] * r_s_ * tint[0] * brightness, base[:, 1] * tint[1] * brightness,
                    base[:, 2] * b_s_ * tint[2] * brightness], axis=-1)
    return np.clip(out, t(0), t(10))


def render(cam, A, sky, tex, h_base=0.1, r_inner=2.0, r_outer=15.0, t_offset=0.0, dtype=np.float64):
    """One frame of the camera `cam` (build_camera): dict with bg, disk, final = clip(bg + disk) as (H, W, 3) in `dtype`,
    fate, n_hits, steps as (H, W), esc_dir and first_hit (H, W, 3 / 2; NaN without one).  ValueError for a camera inside the
    static limit (check_camera), as the library's."""
    t = np.dtype(dtype).type
    check_camera(cam["pos"], A)
    W, H = cam["width"], cam["height"]
    d = pixel_rays(cam, dtype).reshape(-1, 3)
    x0 = cam["pos"].astype(dtype)
    m = march(x0, d, A, h_base, cam["r_escape"], r_inner, r_outer, dtype)
    a = t(A) * t(M)
    n = W * H
    accum = np.zeros((n, 3), dtype=dtype)
    alpha = np.zeros(n, dtype=dtype)
    rows = m["hits"]
    first = np.full((n, 2), np.nan)
    for k in range(int(rows[:, 1].max()) + 1 if rows.shape[0] else 0):       # front to back
        sel = rows[rows[:, 1] == k]
        ray = sel[:, 0].astype(np.int64)
        hx, hy, to_cam = sel[:, 2].astype(dtype), sel[:, 3].astype(dtype), sel[:, 4:7].astype(dtype)
        if k == 0:
            first[ray] = sel[:, 2:4]
        hit_r = np.sqrt(hx * hx + hy * hy - a * a)
        rgba = sample_disk(tex, hx, hy, hit_r, a, r_inner, r_outer, t_offset)
        base_alpha = np.minimum(rgba[:, 3], t(0.999))
        disk_alpha = t(1) - (t(1) - base_alpha) ** t(DISK_ALPHA_GAIN)
        col = g_factor(rgba[:, :3], hx, hy, hit_r, to_cam, a, cam["pos"], r_inner, r_outer)
        front = t(1) - alpha[ray]
        accum[ray] = accum[ray] + col * (disk_alpha * front)[:, None]
        alpha[ray] = t(1) - front * (t(1) - disk_alpha)
    bg = np.zeros((n, 3), dtype=dtype)
    esc = m["fate"] == 1
    if esc.any():
        bg[esc] = sample_skybox(sky, m["esc_dir"][esc].astype(dtype)) * (t(1) - alpha[esc])[:, None]
    disk = np.clip(accum, t(0), t(1))
    sh = (H, W)
    return dict(bg=bg.reshape(H, W, 3), disk=disk.reshape(H, W, 3), final=np.clip(bg + disk, t(0), t(1)).reshape(H, W, 3),
                fate=m["fate"].reshape(sh), n_hits=m["n_hits"].reshape(sh), steps=m["steps"].reshape(sh),
                esc_dir=np.where(esc[:, None], m["esc_dir"], 0.0).reshape(H, W, 3), first_hit=first.reshape(H, W, 2))
