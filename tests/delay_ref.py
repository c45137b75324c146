"""CPU reference of the light delay (include/bhr.h: bhr_render_delayed; DESIGN.md "Light delay"), in NumPy.

Imports nothing from the product.  The stepping is tests/observer_ref.py's Schwarzschild march at beta = 0, statement for statement
(march() below is that loop with the time quadrature beside it; tests/test_delay_ref.py holds the two to the same rays, steps
and hits, exactly); the camera, the samplers, the step factor and the g-factor are imported from kerr_ref and observer_ref.

The model (units r_s = 1, c = 1).  The march integrates x'' = -1.5 L^2 x / r^5 with |d| = 1 at the camera.  Along that parameter
l a null geodesic has E = sqrt(1 - L^2 / r_cam^3) and dt/dl = E w(r), w(r) = r / (r - 1) on r clamped to max(r, 1 + 1e-3).  Per
step from (p, d, r) to (np, nd, rn) under h: m = 0.5 (p + np) + (h / 8)(d - nd), r_m = |m|,
dT = E * h / 6 * (w(r) + 4 w(r_m) + w(rn)); per crossing T_hit = T + t_frac dT; per shade the disk rolls under
t_eff = t_offset - scale * T_hit.  binary64 by default; dtype=np.float32 evaluates every operation in f32 in the device's order
(csrc/ray_delay.h states it rounding by rounding; the exactly rounded sqrt and divide are NumPy's).
"""
import numpy as np

import kerr_ref as K
import observer_ref as R

RS = 1.0
SCALE_MAX = 16.0


def w_of(r):
    """w(r) = r / (r - 1) on the march's r_safe."""
    t = r.dtype.type
    rs = np.maximum(r, t(RS) + t(1e-3))
    return rs / (rs - t(1))


def march(x0, d, h_base=0.1, r_escape=12.0, r_inner=2.0, r_outer=15.0, tilt_deg=0.0, dtype=np.float64):
    """observer_ref.march with the light's coordinate time.  dict: fate, steps, esc_dir, n_hits as there; hits: rows (ray, rank,
    hit_x, hit_y, to_cam xyz, T_hit); T: the time at termination (after the last step), r_end: |p| there, E: the rays' energy."""
    t = np.dtype(dtype).type
    n = d.shape[0]
    p = np.broadcast_to(np.asarray(x0, dtype=dtype), (n, 3)).copy()
    dd = np.asarray(d, dtype=dtype).copy()
    tan_t = t(np.tan(np.float32(np.float32(tilt_deg) * np.float32(np.pi) / np.float32(180.0)).astype(dtype)))
    Lv = np.cross(dd, p)
    Ln = np.sqrt(R._dot(Lv, Lv))
    m15 = t(-1.5) * (Ln * Ln)
    r_esc, hb = t(np.float32(r_escape)), t(np.float32(h_base))
    max_iter = int(np.float32(r_escape) * np.float32(40.0) / np.float32(h_base))
    max_affine = t(np.float32(r_escape) * np.float32(40.0))
    r2 = R._dot(p, p)
    r = np.sqrt(r2)
    # --- the delay's launch
    E = np.sqrt(t(1) - (Ln * Ln) / (r2 * r))
    E_all = E.copy()
    w = w_of(r)
    T = np.zeros(n, dtype=dtype)
    T_end = np.zeros(n, dtype=dtype)
    r_end = r.copy()
    # ---
    f_old = p[:, 2] - p[:, 1] * tan_t
    affine = np.zeros(n, dtype=dtype)
    idx = np.arange(n)
    fate = np.full(n, 2, dtype=np.int8)
    steps = np.zeros(n, dtype=np.int64)
    fin_d = dd.copy()
    n_hits = np.zeros(n, dtype=np.int32)
    hit_rows = []
    half, two, six, four, eighth = t(0.5), t(2), t(6), t(4), t(0.125)

    def acc(s, s2, sr):                    # (-1.5 L^2 / r^5) s, r^5 = (r2 r2) r
        return (m15 / (s2 * s2 * sr))[:, None] * s

    it = 0
    while idx.size and it < max_iter:
        h = (hb * K.dt_fac(r))[:, None]
        k1p = h * dd
        k1d = h * acc(p, r2, r)
        s2 = p + half * k1p
        q2 = R._dot(s2, s2)
        k2p = h * (dd + half * k1d)
        s3 = p + half * k2p
        q3 = R._dot(s3, s3)
        k2d = h * acc(s2, q2, np.sqrt(q2))
        k3p = h * (dd + half * k2d)
        k3d = h * acc(s3, q3, np.sqrt(q3))
        s4 = p + k3p
        q4 = R._dot(s4, s4)
        k4p = h * (dd + k3d)
        k4d = h * acc(s4, q4, np.sqrt(q4))
        np_ = p + (((k1p + two * k2p) + two * k3p) + k4p) / six
        nd = dd + (((k1d + two * k2d) + two * k3d) + k4d) / six
        r2n = R._dot(np_, np_)
        rn = np.sqrt(r2n)
        aff = affine + h[:, 0]
        captured = rn < t(RS)
        ended = captured | (rn > r_esc) | (aff > max_affine)
        f_new = np_[:, 2] - np_[:, 1] * tan_t
        # --- the delay's step: Simpson's rule with the Hermite midpoint
        mid = half * (p + np_) + (eighth * h) * (dd - nd)
        rm = np.sqrt(R._dot(mid, mid))
        wn = w_of(rn)
        dT = (E * (h[:, 0] / six)) * ((w + four * w_of(rm)) + wn)
        # ---
        cross = (f_old * f_new < 0) & ~ended
        if cross.any():
            c = np.nonzero(cross)[0]
            tf = f_old[c] / (f_old[c] - f_new[c] + t(1e-8))
            hx = p[c, 0] + tf * (np_[c, 0] - p[c, 0])
            hy = p[c, 1] + tf * (np_[c, 1] - p[c, 1])
            hr = np.sqrt(hx * hx + hy * hy)
            ok = (t(r_outer) >= hr) & (hr >= t(r_inner))
            t_hit = T[c] + tf * dT[c]
            c, hx, hy, t_hit = c[ok], hx[ok], hy[ok], t_hit[ok]
            if c.size:
                ray = idx[c]
                hit_rows.append(np.column_stack([ray, n_hits[ray], hx, hy, -dd[c, 0], -dd[c, 1], -dd[c, 2], t_hit]))
                n_hits[ray] += 1
        Tn = T + dT
        it += 1
        steps[idx] = it
        T_end[idx] = Tn
        r_end[idx] = rn
        if ended.any():
            e = np.nonzero(ended)[0]
            fate[idx[e]] = np.where(captured[e], 0, 1)
            fin_d[idx[e]] = nd[e]
            keep = ~ended
            idx, p, dd, r, r2, f_old, affine, m15 = idx[keep], np_[keep], nd[keep], rn[keep], r2n[keep], f_new[keep], aff[keep], m15[keep]
            E, w, T = E[keep], wn[keep], Tn[keep]
        else:
            p, dd, r, r2, f_old, affine = np_, nd, rn, r2n, f_new, aff
            w, T = wn, Tn
    if idx.size:
        fin_d[idx] = dd
    rows = np.concatenate(hit_rows) if hit_rows else np.zeros((0, 8))
    return dict(fate=fate, steps=steps, esc_dir=fin_d, hits=rows, n_hits=n_hits, T=T_end, r_end=r_end, E=E_all)


def render(cam, scale, sky, tex, h_base=0.1, r_inner=2.0, r_outer=15.0, tilt_deg=0.0, t_offset=0.0, dtype=np.float64):
    """One frame of the camera `cam` (kerr_ref.build_camera) under the light delay `scale`: dict with bg, disk as (H, W, 3) in
    `dtype`, fate, n_hits, steps as (H, W), T (H, W) at termination, hits: the march's rows, with T_hit in the last column."""
    t = np.dtype(dtype).type
    W, H = cam["width"], cam["height"]
    n_dir = K.pixel_rays(cam, dtype).reshape(-1, 3)
    m = march(cam["pos"].astype(dtype), n_dir, h_base, cam["r_escape"], r_inner, r_outer, tilt_deg, dtype)
    tilt = np.float32(np.float32(tilt_deg) * np.float32(np.pi) / np.float32(180.0)).astype(dtype)
    tan_t, sin_t, cos_t = t(np.tan(tilt)), t(np.sin(tilt)), t(np.cos(tilt))
    n = W * H
    accum = np.zeros((n, 3), dtype=dtype)
    alpha = np.zeros(n, dtype=dtype)
    rows = m["hits"]
    one = np.ones(n, dtype=dtype)
    t_off, sc = t(np.float32(t_offset)), t(np.float32(scale))
    for k in range(int(rows[:, 1].max()) + 1 if rows.shape[0] else 0):       # front to back
        sel = rows[rows[:, 1] == k]
        ray = sel[:, 0].astype(np.int64)
        hx, hy, to_cam = sel[:, 2].astype(dtype), sel[:, 3].astype(dtype), sel[:, 4:7].astype(dtype)
        t_eff = t_off - sc * sel[:, 7].astype(dtype)
        hit_r = np.sqrt(hx * hx + hy * hy)
        rgba = K.sample_disk(tex, hx, hy, hit_r, 0.0, r_inner, r_outer, t_eff)
        base_alpha = np.minimum(rgba[:, 3], t(0.999))
        disk_alpha = t(1) - (t(1) - base_alpha) ** t(K.DISK_ALPHA_GAIN)
        col = R.g_factor(rgba[:, :3], hx, hy, hy * tan_t, hit_r, to_cam, cam["pos"], r_inner, r_outer, sin_t, cos_t, one[ray])
        front = t(1) - alpha[ray]
        accum[ray] = accum[ray] + col * disk_alpha[:, None] * front[:, None]
        alpha[ray] = t(1) - front * (t(1) - disk_alpha)
    bg = np.zeros((n, 3), dtype=dtype)
    esc = m["fate"] == 1
    if esc.any():
        e = m["esc_dir"][esc].astype(dtype)
        e = (t(1) / np.sqrt(R._dot(e, e)))[:, None] * e
        bg[esc] = K.sample_skybox(sky, e) * (t(1) - alpha[esc])[:, None]
    disk = np.clip(accum, t(0), t(1))
    sh = (H, W)
    return dict(bg=bg.reshape(H, W, 3), disk=disk.reshape(H, W, 3), fate=m["fate"].reshape(sh), n_hits=m["n_hits"].reshape(sh),
                steps=m["steps"].reshape(sh), T=m["T"].reshape(sh), hits=rows)


# ----------------------------------------------------------------------------------------------- the independent integration
def geodesic_first_crossing(x0, d, h_base, tilt_deg=0.0, r_inner=2.0, r_outer=15.0, l_max=60.0):
    """Nothing of the march: the four-dimensional Schwarzschild null geodesic in the coordinates x = r n, binary64, plain RK4 at
    the affine step h_base * dt_fac(r) (the march's step rule, so that "ten times finer" holds at every radius), from the Hamiltonian
        H = 1/2 [-p_t^2 / f + |p|^2 - (x.p)^2 / r^3],  f = 1 - 1 / r
    (the inverse of ds^2 = -f dt^2 + dx.dx + (1 / f - 1)(n.dx)^2).  The ray starts at x0 with dx/dlambda = d (one ray, |d| = 1);
    p_t = -E follows from H = 0.  -> (t, x) at the ray's first crossing of the plane z - y tan(tilt) = 0 whose cylindrical radius
    sqrt(x^2 + y^2) lies in [r_inner, r_outer], the crossing located inside its step by secant iterations on partial steps; None if
    there is none within l_max."""
    x = np.asarray(x0, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    tan_t = np.tan(np.radians(tilt_deg))
    r = np.linalg.norm(x)
    nrm = x / r
    f = 1.0 - 1.0 / r
    dr = float(nrm @ d)
    p = (d - dr * nrm) + (dr / f) * nrm                    # dx/dlambda = p - (n.p) n / r
    E = np.sqrt(f * (p @ p - (nrm @ p) ** 2 / r))          # H = 0

    def rhs(y):
        xx, pp = y[1:4], y[4:7]
        rr = np.sqrt(xx @ xx)
        ff = 1.0 - 1.0 / rr
        xp = xx @ pp
        dt = E / ff
        dx = pp - xp * xx / rr ** 3
        dp = -0.5 * (E * E / (ff * ff * rr ** 3) * xx - 2.0 * xp * pp / rr ** 3 + 3.0 * xp * xp * xx / rr ** 5)
        return np.concatenate([[dt], dx, dp])

    def rk4(y, hh):
        k1 = rhs(y)
        k2 = rhs(y + 0.5 * hh * k1)
        k3 = rhs(y + 0.5 * hh * k2)
        k4 = rhs(y + hh * k3)
        return y + hh / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)

    plane = lambda y: y[3] - y[2] * tan_t
    y = np.concatenate([[0.0], x, p])
    lam = 0.0
    while lam < l_max:
        h = h_base * float(K.dt_fac(np.array([np.linalg.norm(y[1:4])]))[0])
        yn = rk4(y, h)
        rn = np.linalg.norm(yn[1:4])
        if rn < 1.0 + 1e-3:
            return None
        f0, f1 = plane(y), plane(yn)
        if f0 * f1 < 0:
            s0, s1, g0, g1 = 0.0, 1.0, f0, f1              # secant on the step fraction
            ys = yn
            for _ in range(8):
                s = s1 - g1 * (s1 - s0) / (g1 - g0)
                ys = rk4(y, s * h)
                g = plane(ys)
                s0, g0, s1, g1 = s1, g1, s, g
                if abs(g) < 1e-15:
                    break
            rc = np.hypot(ys[1], ys[2])
            if r_inner <= rc <= r_outer:
                return float(ys[0]), ys[1:4].copy()
        y = yn
        lam += h
    return None
