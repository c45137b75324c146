"""CPU reference of the Kerr march over the analytic Disk V2 sources (bhr_set_kerr_disk_source; csrc/ray_kerr_dv2.h), in NumPy.

The march is kerr_ref's: initial_momentum, rk4_step, dt_fac, ks_radius, the camera and the sky sampler are imported, not restated.
What is shaded is the Disk V2 model at the Kerr cylinder coordinates of a Kerr-Schild point x with Kerr-Schild radius r:

    varpi = sqrt(max(r^2 - z^2, 0))          on the plane z = 0: sqrt(x^2 + y^2 - a^2), the Boyer-Lindquist hit radius
    zeta  = z,  phi = atan2(y, x),  phi_adv = phi + t_offset omega_field(varpi)          (the model's own pattern speed)

Surface: every crossing kerr_ref's march finds is shaded with T = clamp(t_mid F / t_peak), alpha = clamp(rho_mid F), F =
structure_total(varpi, phi_adv), rgb = dv2_color(T), then kerr_ref.render's opacity, g-factor (kerr_ref.g_factor, or
kerr_redshift_ref's exact one) and front-to-back compositing.
Volume: every step that does not end the ray is one chord x -> x_new cut into `substeps` pieces sampled at their midpoints:
rho = max(rho_field F, 0), T = clamp(t_field F / t_peak), mu = |e_z| / |e|, op = 1 - exp(-Ca rho (1 + kg (1 - mu)) ds), colour
g_factor(dv2_color(T), s_x, s_y, varpi, -dx/dl at the start of the step).  EVERY chord is sampled: there is no cull here.  A ray
stops collecting once its opacity has reached VOLUME_OPAQUE, tested once per chord.

The Disk V2 fields come from oracle.dv2_eval (binary64 C) in binary64 whatever `dtype` is -- the device evaluates them in binary64
from its f32 points too -- and `dtype` is the number format of the march, the g-factor and the compositing.  dv2_color restates
csrc/march_device.h: disk_v2_color; tests/test_kerr_dv2_ref.py checks it against oracle.probe_dv2_rgba.  Nothing here imports the
product package but for the host-side parameter packing (bhr_amd.disk_v2.pack_params: no device).
"""
import numpy as np

import kerr_ref as K
import kerr_redshift_ref as R
from oracle import oracle as O

M = K.M
VOLUME_OPAQUE = 0.9999
F_OMEGA, F_RHO_MID, F_T_MID, F_RHO, F_T, F_SHEAR, F_HOTSPOT, F_TOTAL = 5, 6, 7, 8, 9, 11, 12, 13     # include/bhr_disk_v2.h


class Model:
    """The parameter block and normalisation constants of one Disk V2 disk: what HipRenderer.use_kerr_disk_v2 hands the library,
    made without a device -- bhr_amd.disk_v2.reference_norms' grid, the raw sums from the oracle."""

    def __init__(self, params=None, structure_params=None, seed=42, n_r=512, n_phi=2048):
        from bhr_amd import disk_v2 as dv
        self.params = params or dv.DiskV2Params()
        self.cp = dv.pack_params(self.params, structure_params, shear_seed=seed, hotspot_seed=seed + 1)
        r = np.linspace(self.params.r_in, self.params.r_out, n_r)
        phi = np.linspace(0.0, 2.0 * np.pi, n_phi, endpoint=False)
        rg, pg = np.meshgrid(r, phi, indexing="ij")
        self.norm_shear = float(np.abs(O.dv2_eval(self.cp, F_SHEAR, rg, phi=pg)).max())
        self.norm_hotspot = float(np.abs(O.dv2_eval(self.cp, F_HOTSPOT, rg, phi=pg)).max())
        self.t_peak = float(O.dv2_eval(self.cp, F_T_MID, r).max())

    def field(self, which, r, z=None, phi=None):
        return O.dv2_eval(self.cp, which, r, z=z, phi=phi, norm_shear=self.norm_shear, norm_hotspot=self.norm_hotspot)


def cylinder(x, a):
    """(varpi, zeta, phi) of Kerr-Schild points x (n, 3) around the hole of spin parameter a, in binary64."""
    x = np.asarray(x, dtype=np.float64)
    r = K.ks_radius(x, float(a))
    return np.sqrt(np.maximum(r * r - x[:, 2] * x[:, 2], 0.0)), x[:, 2], np.arctan2(x[:, 1], x[:, 0])


def dv2_color(tf):
    """csrc/march_device.h: disk_v2_color -- the black body of T_K = T_min + tf (T_max - T_min) times sqrt(tf), blue <= red."""
    t = tf.dtype.type
    t_factor = (t(K.DISK_COLOR_TEMPERATURE) - t(4500)) / (t(6500) - t(2700))
    T_min, T_max = t(2000) + t_factor * t(1000), t(9000) + t_factor * t(3000)
    tk = (T_min + tf * (T_max - T_min)) / t(100)
    hot = np.maximum(tk - t(60), t(0.0001))
    cr = np.where(tk > t(66), np.clip(t(1.292936) * hot ** t(-0.1332047592), t(0), t(1)), t(1))
    cg = np.where(tk <= t(66), np.clip(t(0.390082) * np.log(np.maximum(tk, t(0.0001))) - t(0.631841), t(0), t(1)),
                  np.clip(t(1.129891) * hot ** t(-0.0755148492), t(0), t(1)))
    cb_cool = np.where(tk <= t(19), t(0), np.clip(t(0.543207) * np.log(np.maximum(tk - t(10), t(0.0001))) - t(1.19625), t(0), t(1)))
    cb = np.minimum(np.where(tk < t(66), cb_cool, t(1)), cr)
    lum = np.clip(np.sqrt(tf), t(0), t(1))
    return np.clip(np.stack([cr * lum, cg * lum, cb * lum], axis=-1), t(0), t(1)).astype(tf.dtype)


def surface_rgba(model, hx, hy, a, t_offset):
    """disk_v2_rgba's mapping at the Kerr cylinder coordinates of crossings (hx, hy) of the plane: (rgb (n, 3), alpha (n,)) in
    the dtype of hx; the fields in binary64 from those points."""
    dtype = hx.dtype
    x, y, a = hx.astype(np.float64), hy.astype(np.float64), float(a)
    w = np.sqrt(np.maximum(x * x + y * y - a * a, 0.0))
    phi = np.arctan2(y, x) + float(t_offset) * model.field(F_OMEGA, w)
    F = model.field(F_TOTAL, w, phi=phi)
    T = np.clip(model.field(F_T_MID, w) * F / model.t_peak, 0.0, 1.0)
    alpha = np.clip(model.field(F_RHO_MID, w) * F, 0.0, 1.0)
    return dv2_color(T.astype(dtype)), alpha.astype(dtype)


def _frame(cam, sky, m, accum, alpha, dtype):
    t = np.dtype(dtype).type
    W, H = cam["width"], cam["height"]
    bg = np.zeros((W * H, 3), dtype=dtype)
    esc = m["fate"] == 1
    if esc.any():
        bg[esc] = K.sample_skybox(sky, m["esc_dir"][esc].astype(dtype)) * (t(1) - alpha[esc])[:, None]
    disk = np.clip(accum, t(0), t(1))
    return dict(bg=bg.reshape(H, W, 3), disk=disk.reshape(H, W, 3), final=np.clip(bg + disk, t(0), t(1)).reshape(H, W, 3),
                fate=m["fate"].reshape(H, W), n_hits=m["n_hits"].reshape(H, W), steps=m["steps"].reshape(H, W))


def render_surface(cam, A, sky, model, h_base=0.1, r_inner=2.0, r_outer=15.0, t_offset=0.0, redshift="model", dtype=np.float64):
    """kerr_ref.render's frame dict with the Disk V2 surface in the texture's place; redshift "exact": kerr_redshift_ref's g."""
    t = np.dtype(dtype).type
    K.check_camera(cam["pos"], A)
    n = cam["width"] * cam["height"]
    d = K.pixel_rays(cam, dtype).reshape(-1, 3)
    exact = redshift == "exact"
    march = R.march if exact else K.march
    m = march(cam["pos"].astype(dtype), d, A, h_base, cam["r_escape"], r_inner, r_outer, dtype)
    a = t(A) * t(M)
    isco = R.isco_orbit(A) if exact else None
    t_off = float(np.float32(t_offset))
    accum = np.zeros((n, 3), dtype=dtype)
    alpha = np.zeros(n, dtype=dtype)
    rows = m["hits"]
    for k in range(int(rows[:, 1].max()) + 1 if rows.shape[0] else 0):       # front to back
        sel = rows[rows[:, 1] == k]
        ray = sel[:, 0].astype(np.int64)
        hx, hy = sel[:, 2].astype(dtype), sel[:, 3].astype(dtype)
        hit_r = np.sqrt(hx * hx + hy * hy - a * a)
        rgb, al = surface_rgba(model, hx, hy, a, t_off)
        base_alpha = np.minimum(al, t(0.999))
        disk_alpha = t(1) - (t(1) - base_alpha) ** t(K.DISK_ALPHA_GAIN)
        if exact:
            lz, P, U = (sel[:, c].astype(dtype) for c in range(4, 7))
            col = R.shade_g(rgb, R.g_exact(hx, hy, lz, P, U, a, cam["pos"], isco), hit_r, r_inner, r_outer)
        else:
            col = K.g_factor(rgb, hx, hy, hit_r, sel[:, 4:7].astype(dtype), a, cam["pos"], r_inner, r_outer)
        front = t(1) - alpha[ray]
        accum[ray] = accum[ray] + col * (disk_alpha * front)[:, None]
        alpha[ray] = t(1) - front * (t(1) - disk_alpha)
    return _frame(cam, sky, m, accum, alpha, dtype)


def volume_chords(model, x0, x1, v0, a, cam_pos, r_inner, r_outer, t_offset, absorption, grazing_gain, substeps, accum, alpha):
    """Composites the chords x0 -> x1 (n, 3; v0 = dx/dl at x0) onto accum (n, 3) and alpha (n,), in place.  No cull: every piece
    of every chord whose ray is not opaque yet is sampled (a piece of zero density composites nothing)."""
    dtype = x0.dtype
    t = dtype.type
    live = np.nonzero(alpha < t(VOLUME_OPAQUE))[0]
    if not live.size:
        return
    p0, p1 = x0[live].astype(np.float64), x1[live].astype(np.float64)
    e = p1 - p0
    length = np.sqrt((e * e).sum(-1))
    ok = length > 0.0
    live, p0, e, length = live[ok], p0[ok], e[ok], length[ok]
    mu = np.abs(e[:, 2]) / length
    ds = length / float(substeps)
    to_cam = -v0[live]
    for k in range(int(substeps)):
        s = p0 + ((k + 0.5) / float(substeps)) * e
        w, zeta, phi = cylinder(s, a)
        rho0 = model.field(F_RHO, w, z=zeta)
        on = np.nonzero(rho0 > 0.0)[0]                      # (elsewhere rho = 0, op = 0: nothing to composite)
        if not on.size:
            continue
        w, zeta, rho0 = w[on], zeta[on], rho0[on]
        phi = phi[on] + float(t_offset) * model.field(F_OMEGA, w)
        F = model.field(F_TOTAL, w, phi=phi)
        rho = np.maximum(rho0 * F, 0.0)
        T = np.clip(model.field(F_T, w, z=zeta) * F / model.t_peak, 0.0, 1.0)
        op = (1.0 - np.exp(-(absorption * rho * (1.0 + grazing_gain * (1.0 - mu[on]))) * ds[on])).astype(dtype)
        col = K.g_factor(dv2_color(T.astype(dtype)), s[on, 0].astype(dtype), s[on, 1].astype(dtype), w.astype(dtype), to_cam[on], a, cam_pos,
                         r_inner, r_outer)
        ray = live[on]
        pos = op > t(0)
        ray, op, col = ray[pos], op[pos], col[pos]
        front = t(1) - alpha[ray]
        accum[ray] = accum[ray] + col * (op * front)[:, None]
        alpha[ray] = t(1) - front * (t(1) - op)


def render_volume(cam, A, sky, model, h_base=0.1, r_inner=2.0, r_outer=15.0, t_offset=0.0, absorption=4.0, grazing_gain=1.0, substeps=2,
                  dtype=np.float64):
    """The frame dict of the Disk V2 volume around the hole of spin A (model redshift): kerr_ref.march's loop with every step's
    chord integrated instead of its crossing parked (n_hits is 0 everywhere: the volume has no crossings)."""
    t = np.dtype(dtype).type
    K.check_camera(cam["pos"], A)
    n = cam["width"] * cam["height"]
    a = t(A) * t(M)
    x = np.broadcast_to(cam["pos"].astype(dtype), (n, 3)).copy()
    p = K.initial_momentum(x, K.pixel_rays(cam, dtype).reshape(-1, 3), a)
    rp, r_esc, hb = t(K.r_plus(float(A))), t(cam["r_escape"]), t(h_base)
    max_iter = int(np.float32(cam["r_escape"]) * np.float32(40.0) / np.float32(h_base))
    max_affine = t(np.float32(cam["r_escape"]) * np.float32(40.0))
    t_off = float(np.float32(t_offset))
    r = K.ks_radius(x, a)
    affine = np.zeros(n, dtype=dtype)
    idx = np.arange(n)
    fate = np.full(n, 2, dtype=np.int8)
    steps = np.zeros(n, dtype=np.int64)
    fin_x, fin_p = x.copy(), p.copy()
    accum = np.zeros((n, 3), dtype=dtype)
    alpha = np.zeros(n, dtype=dtype)
    it = 0
    while idx.size and it < max_iter:
        h = hb * K.dt_fac(r)
        nx, npm, v1 = K.rk4_step(x, p, h, a)
        rn = K.ks_radius(nx, a)
        aff = affine + h
        captured = rn < rp
        ended = captured | (rn > r_esc) | (aff > max_affine)
        go = np.nonzero(~ended)[0]
        if go.size:
            acc, al = accum[idx[go]], alpha[idx[go]]
            volume_chords(model, x[go], nx[go], v1[go], a, cam["pos"], r_inner, r_outer, t_off, absorption, grazing_gain, substeps, acc, al)
            accum[idx[go]], alpha[idx[go]] = acc, al
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
    m = dict(fate=fate, steps=steps, esc_dir=v / np.sqrt((v * v).sum(-1))[:, None], n_hits=np.zeros(n, dtype=np.int32))
    return _frame(cam, sky, m, accum, alpha, dtype)
