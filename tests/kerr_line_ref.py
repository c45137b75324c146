"""CPU reference of the Kerr line profile (bhr_set_kerr_line; include/bhr.h "Kerr line profile"), in NumPy.

The model, per record (hx, hy, v) of a pixel's front-to-back list:
    r      = sqrt(hx^2 + hy^2 - a^2); the record COUNTS iff r_in <= r <= r_out (the line's annulus) and, under orders "first", no
             earlier record of the pixel counted
    g      exact: kerr_redshift_ref.g_exact of the photon's (L_z, P, U) at the hit; model: kerr_ref.g_factor's own g (g_model)
    dOmega = cos^3 theta, cos theta = D . forward
    eps    = (r / r_in)^-q  [powerlaw]   times  alpha = 1 - (1 - min(A, 0.999))^6 of the disk texture at the crossing  [texture]
    T      = 1 - alpha_total in front of the record, accumulated over every record inside the DISK's annulus as the frame
             composites -- under texture + all only, else 1
    w      = ((g^p eps) dOmega) T
and the histogram: t = (g - g_min) * scale, t < 0 -> under, floor(t) >= n_bins -> over, Q = rint(w * unit) added to the cell, with
scale = f32(n_bins / (g_max - g_min)) and unit = f32(2^32 / 1.5^p); t, w * unit and both factors are f32 whatever `dtype` is,
because they are the device's contract, not its rounding.

F32_DISTANCE_G / _W: the largest |float32 reference - float64 reference| of g (relative) and of w (relative to the frame's
largest w) over the records of tests/test_kerr_line_ref.py's views, spins and modes, measured and asserted there: the bar of
tests/test_gpu_kerr_line.py is four times it.  Measured 4.32e-7 and 6.54e-6 (the latter is the
texture's: an f32 roll angle times 512 texels of a noisy texture).

Everything runs in `dtype`.  Nothing here imports the product package."""
import numpy as np

import kerr_ref as K
import kerr_redshift_ref as R

G_CAP = K.G_FACTOR_CAP
F32_DISTANCE_G = 4.32e-7
F32_DISTANCE_W = 6.54e-6

VIEWS = ((6.0, 0.0, 0.5), (2.5, 2.0, 1.2), (4.0, 3.0, 2.0))
SPINS = (0.0, 0.6, -0.9, 0.998)
MODES = ("model", "exact")
DEFAULTS = dict(n_bins=256, g_range=(0.0, 2.0), index=3.0, power=4.0, emissivity="powerlaw", orders="first", r_inner=None, r_outer=None)


def settings(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def unit_of(power):
    return np.float32(4294967296.0 / (G_CAP ** float(power)))


def scale_of(n_bins, g_range):
    g_min, g_max = np.float32(g_range[0]), np.float32(g_range[1])
    return np.float32(float(n_bins) / (float(g_max) - float(g_min)))


def max_sum_bound(slots=8, width=7680, height=4320):
    """The largest sum a cell can reach: every record of every pixel at Q = 2^32."""
    return slots * width * height * (1 << 32)


# ----------------------------------------------------------------------------------------------- g per record
def g_model(hx, hy, to_cam, a, cam_pos):
    """kerr_ref.g_factor's lines up to its g, cap included."""
    t = hx.dtype.type
    rs = t(K.RS)
    hit_r = np.sqrt(hx * hx + hy * hy - t(a) * t(a))
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
    cos_theta = vx * (ti * to_cam[..., 0]) + vy * (ti * to_cam[..., 1])
    denom = np.maximum(t(1) - beta * cos_theta, t(1e-3))
    g_doppler = t(1) / (gamma * denom)
    grav_num = np.sqrt(np.maximum(t(1) - rs / np.maximum(r_obs, rs + t(1e-3)), t(1e-6)))
    grav_den = np.sqrt(np.maximum(t(1) - rs / np.maximum(r_em, rs + t(1e-3)), t(1e-6)))
    return np.minimum(g_doppler * (grav_num / grav_den), t(K.G_FACTOR_CAP))


def photon_numbers(hx, hy, px, py, a):
    """(L_z, P, U) of the photon (px, py, .) at the hit, as kerr_g_exact forms them."""
    t = hx.dtype.type
    a = t(a)
    r = np.sqrt(hx * hx + hy * hy - a * a)
    irho = t(1) / np.sqrt(hx * hx + hy * hy)
    lz = hx * py - hy * px
    P = (hx * px + hy * py) * irho
    U = t(1) + (r * P - a * lz * irho) * irho
    return lz, P, U


def record_g(hits, valid, A, mode, cam_pos, dtype=np.float64):
    """g of the records `hits` (..., 5) in the device's layout (hx, hy, then to_cam or the photon's momentum), 0 where not valid."""
    t = np.dtype(dtype).type
    a = t(A) * t(K.M)
    h = np.where(valid[..., None], hits, 1.0).astype(dtype)       # a harmless record where there is none
    hx, hy = h[..., 0], h[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "exact":
            lz, P, U = photon_numbers(hx, hy, h[..., 2], h[..., 3], a)
            shape = hx.shape
            g = R.g_exact(hx.ravel(), hy.ravel(), lz.ravel(), P.ravel(), U.ravel(), a, cam_pos, R.isco_orbit(A)).reshape(shape)
        else:
            g = g_model(hx, hy, h[..., 2:5], a, cam_pos)
    return np.where(valid, g, t(0))


# ----------------------------------------------------------------------------------------------- the frame's samples
def frame_samples(cam, hx, hy, g, crossings, A, s, tex=None, t_offset=0.0, r_disk=(2.0, 15.0), dtype=np.float64):
    """The planes g and w, (K, H, W) each, of the records (hx, hy, g) (K, H, W) of a frame with `crossings` (H, W) per pixel; a
    pixel with more crossings than K is on the overflow list and contributes nothing.  Zeros where a record does not count.
    -> dict g, w, counted (bool), overflow_pixels."""
    t = np.dtype(dtype).type
    a = t(A) * t(K.M)
    Kn, H, W = hx.shape
    hx, hy, g = hx.astype(dtype), hy.astype(dtype), g.astype(dtype)
    listed = crossings > Kn
    r_in = t(np.float32(r_disk[0] if s["r_inner"] is None else s["r_inner"]))
    r_out = t(np.float32(r_disk[1] if s["r_outer"] is None else s["r_outer"]))
    d_in, d_out = t(np.float32(r_disk[0])), t(np.float32(r_disk[1]))
    D = K.pixel_rays(cam, dtype)
    ct = (D * cam["forward"].astype(dtype)).sum(-1)
    domega = (ct * ct) * ct
    tex_on, all_on = s["emissivity"] == "texture", s["orders"] == "all"
    p, q = t(np.float32(s["power"])), t(np.float32(s["index"]))
    alpha_total = np.zeros((H, W), dtype=dtype)
    first_done = np.zeros((H, W), dtype=bool)
    g_out, w_out = np.zeros((Kn, H, W), dtype=dtype), np.zeros((Kn, H, W), dtype=dtype)
    counted = np.zeros((Kn, H, W), dtype=bool)
    for c in range(Kn):
        live = (c < crossings) & ~listed
        x, y = np.where(live, hx[c], t(3)), np.where(live, hy[c], t(0))
        r = np.sqrt(x * x + y * y - a * a)
        in_disk = live & (d_out >= r) & (r >= d_in) & ~first_done
        if tex_on:
            rgba = K.sample_disk(tex, x.ravel(), y.ravel(), r.ravel(), a, d_in, d_out, t_offset).reshape(H, W, 4)
            base_alpha = np.minimum(rgba[..., 3], t(0.999))
            disk_alpha = t(1) - (t(1) - base_alpha) ** t(K.DISK_ALPHA_GAIN)
        else:
            disk_alpha = np.ones((H, W), dtype=dtype)
        cnt = in_disk & (r_out >= r) & (r >= r_in)
        eps = (r / r_in) ** (-q)
        if tex_on:
            eps = eps * disk_alpha
        w = ((np.where(cnt, g[c], t(1)) ** p) * eps) * domega
        if tex_on and all_on:
            w = w * (t(1) - alpha_total)
        g_out[c] = np.where(cnt, g[c], t(0))
        w_out[c] = np.where(cnt, w, t(0))
        counted[c] = cnt
        if not all_on:
            first_done = first_done | cnt
        if tex_on:
            front = t(1) - alpha_total
            alpha_total = np.where(in_disk, t(1) - front * (t(1) - disk_alpha), alpha_total)
    return dict(g=g_out, w=w_out, counted=counted, overflow_pixels=int(listed.sum()))


def sample_q(w, power):
    """Q = rint(f32(w) * unit) as uint64: the device's llrintf (round half to even, as np.rint)."""
    return np.rint(np.asarray(w, dtype=np.float32) * unit_of(power)).astype(np.uint64)


def histogram(g, w, counted, s, order=None):
    """(bins (n_bins,), under, over) as Python / NumPy unsigned integers from the samples where `counted`; `order`: a permutation
    of the samples to add them in."""
    gs = np.asarray(g, dtype=np.float32)[counted]
    ws = np.asarray(w, dtype=np.float32)[counted]
    if order is not None:
        gs, ws = gs[order], ws[order]
    n_bins = int(s["n_bins"])
    tt = (gs - np.float32(s["g_range"][0])) * scale_of(n_bins, s["g_range"])
    assert tt.dtype == np.float32
    Q = sample_q(ws, s["power"])
    below = ~(tt >= 0)
    fl = np.floor(np.where(below, np.float32(0), tt))
    above = ~below & (fl >= np.float32(n_bins))
    inside = ~below & ~above
    bins = np.zeros(n_bins, dtype=np.uint64)
    np.add.at(bins, fl[inside].astype(np.int64), Q[inside])
    return bins, np.uint64(Q[below].sum(dtype=np.uint64)), np.uint64(Q[above].sum(dtype=np.uint64))


# ----------------------------------------------------------------------------------------------- records of a host march
def rows_to_planes(rows, n_rays, slots, cols):
    """The rows (ray, rank, ...) of a kerr_ref / kerr_redshift_ref march as planes (slots, n_rays, len(cols)) and the count per ray."""
    out = np.zeros((slots, n_rays, len(cols)))
    count = np.zeros(n_rays, dtype=np.int32)
    if rows.shape[0]:
        ray, rank = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)
        np.add.at(count, ray, 1)
        keep = rank < slots
        out[rank[keep], ray[keep]] = rows[keep][:, cols]
    return out, count


def host_records(view, A, mode, width=64, height=36, fov=90.0, slots=4):
    """The records of a binary64 host march of the view in the device's layout, rounded to f32 as the device stores them:
    -> (cam, hits (slots, H, W, 5) float32, crossings (H, W)).  The exact redshift's photon is given as one (px, py, 0) with
    the march's (L_z, P) -- which is all kerr_g_exact takes of it."""
    cam = K.build_camera(view, fov, width, height)
    d = K.pixel_rays(cam).reshape(-1, 3)
    x0 = cam["pos"].astype(np.float64)
    n = width * height
    if mode == "exact":
        m = R.march(x0, d, A, 0.1, cam["r_escape"])
        pl, count = rows_to_planes(m["hits"], n, slots, [2, 3, 4, 5])
        hx, hy, lz, P = (pl[..., k] for k in range(4))
        rho2 = np.where(hx * hx + hy * hy > 0, hx * hx + hy * hy, 1.0)
        rho = np.sqrt(rho2)
        px, py = (hx * P * rho - hy * lz) / rho2, (hy * P * rho + hx * lz) / rho2
        hits = np.stack([hx, hy, px, py, np.zeros_like(px)], axis=-1)
    else:
        m = K.march(x0, d, A, 0.1, cam["r_escape"])
        hits, count = rows_to_planes(m["hits"], n, slots, [2, 3, 4, 5, 6])
    return cam, hits.reshape(slots, height, width, 5).astype(np.float32), count.reshape(height, width)


def frame(cam, hits, crossings, A, mode, s, tex=None, t_offset=0.0, r_disk=(2.0, 15.0), dtype=np.float64):
    """record_g, then frame_samples: the reference's planes of a frame from records in the device's layout."""
    Kn = hits.shape[0]
    valid = (np.arange(Kn)[:, None, None] < np.minimum(crossings, Kn)[None]) & (crossings <= Kn)[None]
    g = record_g(hits, valid, A, mode, cam["pos"], dtype)
    return frame_samples(cam, hits[..., 0], hits[..., 1], g, crossings, A, s, tex, t_offset, r_disk, dtype)
