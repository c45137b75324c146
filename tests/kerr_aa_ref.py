"""CPU reference of the Kerr anti-aliasing (bhr_set_kerr_anti_alias; csrc/ray_kerr.h "Ray differentials"), in NumPy, on top of
tests/kerr_ref.py.

Model.  Beside (x, p) a ray carries two tangents (xi, pi) = d(x, p) / d(pixel), one per pixel axis.  They are integrated by the
same RK4 step with the same h -- h is a constant of the step, as in the reference's variational pair -- through the variational
equations of the system, which are kerr_ref.rhs differentiated line by line in forward mode (`rhs_tangent`):

    dw = 2 x.xi,  dS = (w dw + 4 a^2 z xi_z) / S,  d(r^2) = (dw + dS) / 2,  dr = d(r^2) / (2 r),  d(1/S) = -dS / S^2,
    dQ = d(r^2),  d(1/Q) = -dQ / Q^2,  df = dr / S - r dS / S^2,  dl,  du = dl.p + l.pi,  dv = pi - d(f u) l - f u dl,
    and on through gr, gf, N, dr, gl and dp.

Seeds (`seed_tangent`): xi = 0; with the direction differential dd of the pixel (the direction through the next pixel less the
pixel's own, `pixel_rays_diff`) and f, l constants of the camera,

    dc = l.dd,  ds = -s^3 f c dc,  dLam = (c ds + s dc) / (1 - f),  pi = ds d + s dd + f dLam l.

Hit differentials: the x and y components of the two NEW xi at the end of the crossing step, not projected onto the plane (the
reference's convention).  LOD (`lod_of`): the reference's lines in the Kerr texture coordinates phi = atan2(hy, hx) and the
Boyer-Lindquist r = sqrt(hx^2 + hy^2 - a^2), so dr = (hx xi_x + hy xi_y) / r, with the reference's 1e-6 guards; the roll's own
derivative is ignored.  Level: min(int(clamp(lod strength, 0, 3)), mip_last).  Sampler (`sample_disk_level`): kerr_ref.sample_disk
with the level's size in u, v, the wrap and the clamp.  The g-factor (both redshifts) and the compositing are unchanged.

Everything runs in `dtype` (float64, or float32 to measure what the number format costs).  Nothing here imports the product."""
import numpy as np

import kerr_ref as K

M = K.M
NUM_MIP_LEVELS = 5          # the chain holds the texture and at most four halvings; the LOD never asks beyond level 3


# ----------------------------------------------------------------------------------------------- the variational equations
def rhs_tangent(x, p, xi, pi, a):
    """(d(dx/dl), d(dp/dl)) of kerr_ref.rhs at (x, p) along (xi, pi); xi, pi may carry leading axes in front of x's."""
    t = x.dtype.type
    a = t(a)
    a2 = a * a
    X, Y, Z = x[..., 0], x[..., 1], x[..., 2]
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    ex, ey, ez = xi[..., 0], xi[..., 1], xi[..., 2]
    qx, qy, qz = pi[..., 0], pi[..., 1], pi[..., 2]
    # the primal, as kerr_ref.rhs has it
    w = (X * X + Y * Y + Z * Z) - a2
    S = np.sqrt(w * w + t(4) * a2 * (Z * Z))
    r2 = t(0.5) * (w + S)
    r = np.sqrt(r2)
    iS, ir, Q = t(1) / S, t(1) / r, r2 + a2
    iQ = t(1) / Q
    f = r * iS
    lx, ly, lz = (r * X + a * Y) * iQ, (r * Y - a * X) * iQ, Z * ir
    u = t(1) + (lx * px + ly * py + lz * pz)
    fu = f * u
    g = ir * iS
    grx, gry, grz = r2 * X * g, r2 * Y * g, Q * Z * g
    w2 = t(2) * w
    w4 = w2 + t(4) * a2
    gSx, gSy, gSz = w2 * X * iS, w2 * Y * iS, w4 * Z * iS
    gfx, gfy, gfz = (grx - f * gSx) * iS, (gry - f * gSy) * iS, (grz - f * gSz) * iS
    sxy = X * px + Y * py
    N = r * sxy + a * (Y * px - X * py)
    dr_ = sxy * iQ - t(2) * r * N * iQ * iQ - Z * pz * ir * ir
    glx, gly, glz = (r * px - a * py) * iQ + dr_ * grx, (a * px + r * py) * iQ + dr_ * gry, pz * ir + dr_ * grz
    c1 = t(0.5) * u * u
    # the tangent, line by line
    dw = t(2) * (X * ex + Y * ey + Z * ez)
    dS = (w * dw + t(4) * a2 * Z * ez) * iS
    dr2 = t(0.5) * (dw + dS)                       # = dQ
    dr = t(0.5) * dr2 * ir
    diS = -dS * iS * iS
    diQ = -dr2 * iQ * iQ
    dir_ = -dr * ir * ir
    df = dr * iS + r * diS
    dlx = (dr * X + r * ex + a * ey - lx * dr2) * iQ
    dly = (dr * Y + r * ey - a * ex - ly * dr2) * iQ
    dlz = (ez - lz * dr) * ir
    du = (dlx * px + dly * py + dlz * pz) + (lx * qx + ly * qy + lz * qz)
    dfu = df * u + f * du
    tv = np.stack([qx - dfu * lx - fu * dlx, qy - dfu * ly - fu * dly, qz - dfu * lz - fu * dlz], axis=-1)
    dg = dir_ * iS + ir * diS
    dgrx = (dr2 * X + r2 * ex) * g + r2 * X * dg
    dgry = (dr2 * Y + r2 * ey) * g + r2 * Y * dg
    dgrz = (dr2 * Z + Q * ez) * g + Q * Z * dg
    dw2 = t(2) * dw
    dgSx = (dw2 * X + w2 * ex) * iS + w2 * X * diS
    dgSy = (dw2 * Y + w2 * ey) * iS + w2 * Y * diS
    dgSz = (dw2 * Z + w4 * ez) * iS + w4 * Z * diS
    dgfx = (dgrx - df * gSx - f * dgSx - gfx * dS) * iS
    dgfy = (dgry - df * gSy - f * dgSy - gfy * dS) * iS
    dgfz = (dgrz - df * gSz - f * dgSz - gfz * dS) * iS
    dsxy = ex * px + X * qx + ey * py + Y * qy
    dN = dr * sxy + r * dsxy + a * (ey * px + Y * qx - ex * py - X * qy)
    ddr = (dsxy * iQ + sxy * diQ - t(2) * (dr * N + r * dN) * iQ * iQ - t(4) * r * N * iQ * diQ
           - (ez * pz + Z * qz) * ir * ir - t(2) * Z * pz * ir * dir_)
    dglx = (dr * px + r * qx - a * qy) * iQ + (r * px - a * py) * diQ + ddr * grx + dr_ * dgrx
    dgly = (a * qx + dr * py + r * qy) * iQ + (a * px + r * py) * diQ + ddr * gry + dr_ * dgry
    dglz = qz * ir + pz * dir_ + ddr * grz + dr_ * dgrz
    dc1 = u * du
    tdp = np.stack([dc1 * gfx + c1 * dgfx + dfu * glx + fu * dglx, dc1 * gfy + c1 * dgfy + dfu * gly + fu * dgly,
                    dc1 * gfz + c1 * dgfz + dfu * glz + fu * dglz], axis=-1)
    return tv, tdp


def seed_tangent(x, d, dd, a):
    """pi of the camera's photon under d -> d + dd (xi = 0): the differential of kerr_ref.initial_momentum, f and l constant."""
    t = x.dtype.type
    _, f, l = K.geometry(x, a)
    c = (l * d).sum(-1)
    s = t(1) / np.sqrt(t(1) - f * (t(1) - c * c))
    dc = (l * dd).sum(-1)
    ds = -(s * s * s) * f * c * dc
    dlam = (c * ds + s * dc) / (t(1) - f)
    return ds[..., None] * d + s[..., None] * dd + (f * dlam)[..., None] * l


def rk4_step_tangent(x, p, xi, pi, h, a):
    """kerr_ref.rk4_step on (x, p) and, with the same h, on the tangents (xi, pi) with leading axes; also dx/dl at the start."""
    t = x.dtype.type
    hh = h[..., None]
    half = t(0.5)
    v1, a1 = K.rhs(x, p, a)
    t1, b1 = rhs_tangent(x, p, xi, pi, a)
    x2, p2 = x + half * hh * v1, p + half * hh * a1
    v2, a2_ = K.rhs(x2, p2, a)
    t2, b2 = rhs_tangent(x2, p2, xi + half * hh * t1, pi + half * hh * b1, a)
    x3, p3 = x + half * hh * v2, p + half * hh * a2_
    v3, a3 = K.rhs(x3, p3, a)
    t3, b3 = rhs_tangent(x3, p3, xi + half * hh * t2, pi + half * hh * b2, a)
    x4, p4 = x + hh * v3, p + hh * a3
    v4, a4 = K.rhs(x4, p4, a)
    t4, b4 = rhs_tangent(x4, p4, xi + hh * t3, pi + hh * b3, a)
    six = t(1) / t(6)
    nx = x + hh * ((v1 + t(2) * v2 + t(2) * v3 + v4) * six)
    npm = p + hh * ((a1 + t(2) * a2_ + t(2) * a3 + a4) * six)
    nxi = xi + hh * ((t1 + t(2) * t2 + t(2) * t3 + t4) * six)
    npi = pi + hh * ((b1 + t(2) * b2 + t(2) * b3 + b4) * six)
    return nx, npm, nxi, npi, v1


# ----------------------------------------------------------------------------------------------- camera
def pixel_rays_diff(cam, dtype=np.float64, offset=(0.0, 0.0)):
    """(d, ddx, ddy), each (H, W, 3): kerr_ref.pixel_rays' unit directions and the direction differentials of the pinhole -- the
    unit direction through the pixel one to the right / one below, less the pixel's own.  offset: the rays of the pixel centres
    moved by that many pixels (right, down)."""
    t = np.dtype(dtype).type
    W, H = cam["width"], cam["height"]
    cp, cr, cu, cf = (cam[k].astype(dtype) for k in ("pos", "right", "up", "forward"))
    pw, ph = t(cam["pw"]), t(cam["ph"])
    center = cp + cf
    half_w, half_h = pw * t(W) / t(2), ph * t(H) / t(2)
    tl = (center - half_w * cr) + half_h * cu
    i = np.arange(W, dtype=dtype)[None, :, None] + t(offset[0])
    j = np.arange(H, dtype=dtype)[:, None, None] + t(offset[1])

    def unit(di, dj):
        pos = (tl + ((i + t(di)) * pw) * cr) - ((j + t(dj)) * ph) * cu
        d = pos - cp
        return (t(1) / np.sqrt((d * d).sum(-1)))[..., None] * d
    d = unit(0.5, 0.5)
    return d, unit(1.5, 0.5) - d, unit(0.5, 1.5) - d


# ----------------------------------------------------------------------------------------------- the march
def march(x0, d, dd, A, h_base=0.1, r_escape=12.0, r_inner=2.0, r_outer=15.0, dtype=np.float64, record=False, h_given=None):
    """kerr_ref.march with the two tangents beside each ray.  dd: (2, n, 3), the direction differentials of the two pixel axes.
    The rows of `hits` are (ray, rank, hx, hy, to_cam x y z, dxx, dxy, dyx, dyy, L_z, P, U): kerr_ref's seven, the hit
    differentials (x and y of the two new xi at the end of the crossing step) and kerr_redshift_ref's photon numbers.
    record: also `path`, a list per step of (ray indices, h, new x, new xi) of the rays alive in it.  h_given: a list of per-step
    arrays (n,) of step sizes to take instead of the step rule's (a ray marched with another ray's recorded sequence)."""
    t = np.dtype(dtype).type
    a = t(A) * t(M)
    n = d.shape[0]
    x = np.broadcast_to(np.asarray(x0, dtype=dtype), (n, 3)).copy()
    dirs = np.asarray(d, dtype=dtype)
    p = K.initial_momentum(x, dirs, a)
    pi = seed_tangent(x[None], dirs[None], np.asarray(dd, dtype=dtype), a)
    xi = np.zeros_like(pi)
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
    hit_rows, path = [], []
    it = 0
    while idx.size and it < max_iter and (h_given is None or it < len(h_given)):
        h = hb * K.dt_fac(r) if h_given is None else np.asarray(h_given[it], dtype=dtype)[idx]
        nx, npm, nxi, npi, v1 = rk4_step_tangent(x, p, xi, pi, h, a)
        rn = K.ks_radius(nx, a)
        aff = affine + h
        captured = rn < rp
        ended = captured | (rn > r_esc) | (aff > max_affine)
        if record:
            path.append((idx.copy(), h.copy(), nx.copy(), nxi.copy()))
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
                hit_rows.append(np.column_stack([ray, n_hits[ray], hx, hy, -v1[c, 0], -v1[c, 1], -v1[c, 2],
                                                 nxi[0, c, 0], nxi[0, c, 1], nxi[1, c, 0], nxi[1, c, 1], lz, P, U]))
                n_hits[ray] += 1
        it += 1
        steps[idx] = it
        if ended.any():
            e = np.nonzero(ended)[0]
            fate[idx[e]] = np.where(captured[e], 0, 1)
            fin_x[idx[e]], fin_p[idx[e]] = nx[e], npm[e]
            keep = ~ended
            idx, x, p, r, affine = idx[keep], nx[keep], npm[keep], rn[keep], aff[keep]
            xi, pi = nxi[:, keep], npi[:, keep]
        else:
            x, p, r, affine, xi, pi = nx, npm, rn, aff, nxi, npi
    if idx.size:
        fin_x[idx], fin_p[idx] = x, p
    v, _ = K.rhs(fin_x, fin_p, a)
    esc = v / np.sqrt((v * v).sum(-1))[:, None]
    rows = np.concatenate(hit_rows) if hit_rows else np.zeros((0, 14))
    out = dict(fate=fate, steps=steps, esc_dir=esc, hits=rows, n_hits=n_hits, x=fin_x, p=fin_p)
    if record:
        out["path"] = path
    return out


# ----------------------------------------------------------------------------------------------- shading
def build_mips(tex, levels=NUM_MIP_LEVELS):
    """The mip chain of a disk texture (n_r, n_phi, 4), float32: each level the 2 x 2 box mean of the one before, halved while
    both sides are at least 2, `levels` at the most."""
    mips = [np.asarray(tex, dtype=np.float32)]
    while len(mips) < levels and mips[-1].shape[0] >= 2 and mips[-1].shape[1] >= 2:
        m = mips[-1]
        h, w = m.shape[0] // 2, m.shape[1] // 2
        m = m[:2 * h, :2 * w]
        mips.append(((m[0::2, 0::2] + m[1::2, 0::2] + m[0::2, 1::2] + m[1::2, 1::2]) / np.float32(4)).astype(np.float32))
    return mips


def lod_of(hx, hy, dxx, dxy, dyx, dyy, a, n_r, n_phi, r_inner, r_outer, strength):
    """The LOD of crossings (before the clamp and the truncation): log2(max(|d(u, v)/dx|^2, |d(u, v)/dy|^2, 1)) strength."""
    t = hx.dtype.type
    rho2 = hx * hx + hy * hy
    r_g = np.sqrt(rho2 - t(a) * t(a) + t(1e-6))
    r_cyl = np.sqrt(rho2 + t(1e-6))
    den = r_cyl * r_cyl + t(1e-6)
    w_f, h_f, span = t(n_phi), t(n_r), t(r_outer) - t(r_inner)
    two_pi = t(2) * t(np.float32(np.pi))
    dudx = (-hy * dxx + hx * dxy) / den * w_f / two_pi
    dvdx = (hx * dxx + hy * dxy) / r_g * h_f / span
    dudy = (-hy * dyx + hx * dyy) / den * w_f / two_pi
    dvdy = (hx * dyx + hy * dyy) / r_g * h_f / span
    grad_sq = np.maximum(dudx * dudx + dvdx * dvdx, dudy * dudy + dvdy * dvdy)
    return np.log(np.maximum(grad_sq, t(1))) / np.log(t(2)) * t(strength)


def level_of(lod, mip_last):
    return np.minimum(np.clip(lod, 0, 3).astype(np.int64), mip_last)


def sample_disk_level(mips, level, hx, hy, hit_r, a, r_inner, r_outer, t_offset):
    """kerr_ref.sample_disk at a mip level per crossing: u, v, the wrap and the clamp on the level's size."""
    t = hx.dtype.type
    n_r, n_phi = mips[0].shape[:2]
    two_pi = t(np.float32(2 * np.pi))
    phi = np.arctan2(hy, hx)
    r_safe = np.maximum(hit_r, t(1e-3))
    phi = phi + t(t_offset) * K.omega_kerr(r_safe, a)
    phi = np.mod(phi, two_pi)
    phi = np.where(phi >= two_pi, phi - two_pi, phi)
    out = np.zeros((hx.shape[0], 4), dtype=hx.dtype)
    for lv in np.unique(level):
        m = level == lv
        tex = mips[int(lv)].astype(hx.dtype)
        scale = t(1 << int(lv))
        w_lod, h_lod = t(n_phi) / scale, t(n_r) / scale
        u = phi[m] / two_pi * w_lod
        v = (hit_r[m] - t(r_inner)) / (t(r_outer) - t(r_inner)) * h_lod
        u0, v0 = np.floor(u), np.floor(v)
        fu, fv = (u - u0)[:, None], (v - v0)[:, None]
        u0, v0 = u0.astype(np.int64), v0.astype(np.int64)
        wl, vmax = int(w_lod), int(h_lod - t(1))
        u0w, u1w = np.mod(u0, wl), np.mod(u0 + 1, wl)
        v0h, v1h = np.clip(v0, 0, vmax), np.clip(v0 + 1, 0, vmax)
        one = t(1)
        out[m] = (tex[v0h, u0w] * (one - fu) * (one - fv) + tex[v0h, u1w] * fu * (one - fv) + tex[v1h, u0w] * (one - fu) * fv
                  + tex[v1h, u1w] * fu * fv)
    return out


def render(cam, A, sky, tex, strength=1.0, redshift="model", h_base=0.1, r_inner=2.0, r_outer=15.0, t_offset=0.0, dtype=np.float64):
    """kerr_ref.render's frame dict with the Kerr anti-aliasing at `strength`, under the model or the exact redshift; also
    `lods`: the rows (ray, rank, lod before the clamp) of the shaded crossings, and `max_rank`."""
    t = np.dtype(dtype).type
    K.check_camera(cam["pos"], A)
    W, H = cam["width"], cam["height"]
    d, ddx, ddy = pixel_rays_diff(cam, dtype)
    m = march(cam["pos"].astype(dtype), d.reshape(-1, 3), np.stack([ddx.reshape(-1, 3), ddy.reshape(-1, 3)]), A, h_base,
              cam["r_escape"], r_inner, r_outer, dtype)
    a = t(A) * t(M)
    mips = build_mips(tex)
    mip_last = len(mips) - 1
    n_r, n_phi = mips[0].shape[:2]
    if redshift == "exact":
        import kerr_redshift_ref as R
        isco = R.isco_orbit(A)
    n = W * H
    accum = np.zeros((n, 3), dtype=dtype)
    alpha = np.zeros(n, dtype=dtype)
    rows = m["hits"]
    lods = []
    for k in range(int(rows[:, 1].max()) + 1 if rows.shape[0] else 0):       # front to back
        sel = rows[rows[:, 1] == k]
        ray = sel[:, 0].astype(np.int64)
        hx, hy = sel[:, 2].astype(dtype), sel[:, 3].astype(dtype)
        to_cam = sel[:, 4:7].astype(dtype)
        dxx, dxy, dyx, dyy = (sel[:, c].astype(dtype) for c in range(7, 11))
        hit_r = np.sqrt(hx * hx + hy * hy - a * a)
        lod = lod_of(hx, hy, dxx, dxy, dyx, dyy, a, n_r, n_phi, r_inner, r_outer, strength)
        lods.append(np.column_stack([ray, np.full(ray.shape, k), lod]))
        rgba = sample_disk_level(mips, level_of(lod, mip_last), hx, hy, hit_r, a, r_inner, r_outer, t_offset)
        base_alpha = np.minimum(rgba[:, 3], t(0.999))
        disk_alpha = t(1) - (t(1) - base_alpha) ** t(K.DISK_ALPHA_GAIN)
        if redshift == "exact":
            lz, P, U = (sel[:, c].astype(dtype) for c in range(11, 14))
            col = R.shade_g(rgba[:, :3], R.g_exact(hx, hy, lz, P, U, a, cam["pos"], isco), hit_r, r_inner, r_outer)
        else:
            col = K.g_factor(rgba[:, :3], hx, hy, hit_r, to_cam, a, cam["pos"], r_inner, r_outer)
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
                lods=np.concatenate(lods) if lods else np.zeros((0, 3)))


def near_jump(lods, shape, delta):
    """(H, W) bool: the pixels with a shaded crossing whose lod lies within delta of 1, 2 or 3, where the level jumps."""
    lod = lods[:, 2]
    near = (np.abs(lod - 1) <= delta) | (np.abs(lod - 2) <= delta) | (np.abs(lod - 3) <= delta)
    out = np.zeros(shape[0] * shape[1], dtype=bool)
    out[lods[near, 0].astype(np.int64)] = True
    return out.reshape(shape)
