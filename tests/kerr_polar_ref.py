"""CPU reference of the Kerr polarisation (include/bhr.h "Kerr polarisation"; DESIGN 4 "Kerr polarisation"; no test functions).

Units r_s = 1, M = 1/2, a = A M, the Kerr-Schild chart of kerr_ref (g = eta + f l l, l_mu = (1, l)), the traced photon with
covariant momentum (-1, p) and contravariant k = (1 + f u, p - f u l), u = 1 + l.p.  Four pieces:
  * ``kappa``: the two conserved numbers of a photon k and a polarisation f at a point,
        kappa1 = k^t (x.f) - f^t (x.k) + a (k^x f^y - k^y f^x),   kappa2 = x.(k x f) - a (k^t f^z - k^z f^t);
  * ``crossing_stokes``: the model per stored crossing in NumPy, dtype float64 or float32 (every operation then rounds to f32,
    as the kernel's does), written the way csrc/march_kerr_polar.hip writes it;
  * ``transport``: a binary64 RK4 integrator of the geodesic (kerr_ref.rhs) and the parallel transport
    df^mu/dl = -Gamma^mu_ab k^a f^b with Gamma from central differences of the 4 x 4 metric -- it knows nothing of kappa;
  * ``march_records``: kerr_ref's march keeping, per crossing, the hit point and the photon's whole momentum there -- records
    like the map's, made without a device.
Imports kerr_ref and kerr_redshift_ref only.
"""
import numpy as np

import kerr_ref as K
import kerr_redshift_ref as R

# The largest |Q/I| or |U/I| distance of the float32 evaluation of crossing_stokes from the binary64 one on the records of the
# test views (tests/test_kerr_polar_ref.py measures it and asserts it stays below this); the device's bar is 4 x this.
F32_DISTANCE = 2.08e-6
# ... and of the A = 0 model from polar_ref.crossing_stokes on the same records (the record's own to_cam): the camera stretch the
# Schwarzschild pass ignores and the ray's bend across the crossing's step
SCHWARZSCHILD_DISTANCE = 0.2233


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _unit3(v):
    return v / np.sqrt(_dot3(v, v))[..., None]


def kappa(x, kt, kv, ft, fv, a):
    """(kappa1, kappa2) at x (..., 3) of k = (kt, kv) and f = (ft, fv), contravariant Kerr-Schild components; ``a`` broadcasts."""
    k1 = (kt * _dot3(x, fv) - ft * _dot3(x, kv)) + a * (kv[..., 0] * fv[..., 1] - kv[..., 1] * fv[..., 0])
    k2 = _dot3(x, _cross3(kv, fv)) - a * (kt * fv[..., 2] - kv[..., 2] * ft)
    return k1, k2


def photon_up(x, p, a):
    """The contravariant k = (k^t, k) of the photon with covariant momentum (-1, p) at x."""
    _, f, l = K.geometry(x, a)
    u = 1 + _dot3(l, p)
    return 1 + f * u, p - (f * u)[..., None] * l


def image_axes(cam, D, dtype=np.float64):
    """The Schwarzschild pass's sky-plane axes (e_x, e_y) of the launch directions D (..., 3)."""
    t = dtype
    Rv, U = np.asarray(cam["right"], dtype=t), np.asarray(cam["up"], dtype=t)
    Rb = np.broadcast_to(Rv, D.shape)
    ex = _unit3(Rb - _dot3(Rb, D)[..., None] * D)
    ey = _cross3(D, ex)
    ey = np.where((_dot3(ey, np.broadcast_to(U, D.shape)) < 0)[..., None], -ey, ey)
    return ex, ey


def camera_side(cam, D, a, dtype=np.float64):
    """Per launch direction: p_c (Ray::init's closed form), k_c = (kt, kv), the lifted axes E = (p_c.e, e) and their kappa's.
    -> dict(pc, kt, kv, ex, ey, Ext, Eyt, k1x, k2x, k1y, k2y)."""
    t = dtype
    a = t(a)
    a2 = a * a
    D = np.asarray(D, dtype=t)
    C = np.asarray(cam["pos"], dtype=t)
    w = _dot3(C, C) - a2
    S = np.sqrt(w * w + t(4) * a2 * (C[2] * C[2]))
    r2 = t(0.5) * (w + S)
    r = np.sqrt(r2)
    f, Q = r / S, r2 + a2
    l = np.array([(r * C[0] + a * C[1]) / Q, (r * C[1] - a * C[0]) / Q, C[2] / r], dtype=t)
    c = _dot3(np.broadcast_to(l, D.shape), D)
    sc = t(1) / np.sqrt(t(1) - f * (t(1) - c * c))
    lam = (t(1) + sc * c) / (t(1) - f)
    fl = f * lam
    pc = sc[..., None] * D + fl[..., None] * l
    kt, kv = t(1) + fl, sc[..., None] * D
    ex, ey = image_axes(cam, D, t)
    Cb = np.broadcast_to(C, D.shape)
    Ext, Eyt = _dot3(pc, ex), _dot3(pc, ey)
    k1x, k2x = kappa(Cb, kt, kv, Ext, ex, a)
    k1y, k2y = kappa(Cb, kt, kv, Eyt, ey, a)
    return dict(pc=pc, kt=kt, kv=kv, ex=ex, ey=ey, Ext=Ext, Eyt=Eyt, k1x=k1x, k2x=k2x, k1y=k1y, k2y=k2y)


def _gdot(g, A, B):
    f, lx, ly = g
    la = A[0] + (lx * A[1] + ly * A[2])
    lb = B[0] + (lx * B[1] + ly * B[2])
    return (A[1] * B[1] + A[2] * B[2] - A[0] * B[0]) + f * (la * lb)


def _axpy(s, A, B):
    return tuple(s * x + y for x, y in zip(A, B))


def _gunit(g, A):
    s = 1 / np.sqrt(_gdot(g, A, A))
    return tuple(s * x for x in A)


def gas_velocity(g, hx, hy, r, rho2, irho, a, mode, isco, dtype=np.float64):
    """The gas's 4-velocity (t, x, y) at hits in the plane, the kernel's gas_velocity: ``mode`` "model" or "exact"; isco =
    (r_isco, E, L) of kerr_redshift_ref.isco_orbit (the exact mode's)."""
    t = dtype
    f, lx, ly = g
    zero = np.zeros_like(hx)
    if mode == "exact":
        r_isco, E, L = (t(v) for v in isco)
        om = K.omega_kerr(r, a)
        q = t(1) - a * om
        ut = t(1) / np.sqrt(np.maximum(t(1) - om * om * rho2 - q * q / r, t(1e-6)))
        circ = (ut, -(ut * om) * hy, (ut * om) * hx)
        with np.errstate(all="ignore"):
            w, S = R.plunge_velocity(r, a, r_isco, E, L)
            lr, wr, fs = L / rho2, w * irho, f * S
            plunge = (E + fs, (wr * hx - lr * hy) - fs * lx, (wr * hy + lr * hx) - fs * ly)
        out = r >= r_isco
        return tuple(np.where(out, c, p) for c, p in zip(circ, plunge))
    r_safe = np.maximum(r, t(1) + t(1e-3))
    omega = K.omega_kerr(r_safe, a)
    lorentz = np.sqrt(np.maximum(t(1) - t(1) / r_safe, t(1e-6)))
    beta = np.minimum(r_safe * omega / np.maximum(lorentz, t(1e-6)), t(0.99))
    gamma = t(1) / np.sqrt(np.maximum(t(1) - beta * beta, t(1e-6)))
    us = (t(1) / np.sqrt(np.maximum(t(1) - f, t(1e-6))), zero, zero)
    m = (zero, -hy * irho, hx * irho)
    e = _gunit(g, _axpy(_gdot(g, m, us), us, m))
    return (gamma * (us[0] + beta * e[0]), gamma * (beta * e[1]), gamma * (beta * e[2]))


def crossing_stokes(cam, D, hx, hy, ph, A, mode, field, fraction, r_inner, r_outer, dtype=np.float64, details=False):
    """The model per crossing.  ``D`` (..., 3) launch directions, ``hx``, ``hy`` (...) hit point, ``ph`` (..., 3) the photon's
    covariant momentum there, broadcastable to one shape; ``A`` the spin a / M, ``mode`` "model" or "exact".
    -> (aq, bu, ok): aq = p cos 2chi, bu = p sin 2chi (0 where not ok); ok = the crossing lies in the annulus (the device's
    own f32 test), the pixel's 2 x 2 system is regular, s2 > 0 and alpha^2 + beta^2 > 0.  ``details``: also a dict."""
    t = dtype
    A32 = np.float32(A)
    a = t(np.float32(0.5 * float(A32)))                     # the kernel's kerr_a: binary64 half of the f32 spin, rounded once
    D = np.asarray(D, dtype=t)
    hx, hy = np.asarray(hx, dtype=t), np.asarray(hy, dtype=t)
    ph = np.asarray(ph, dtype=t)
    shape = np.broadcast_shapes(D.shape[:-1], hx.shape, ph.shape[:-1])
    D = np.broadcast_to(D, shape + (3,))
    hx, hy = np.broadcast_to(hx, shape), np.broadcast_to(hy, shape)
    ph = np.broadcast_to(ph, shape + (3,))
    isco = tuple(float(np.float32(v)) for v in R.isco_orbit(float(A32))) if mode == "exact" else None
    with np.errstate(all="ignore"):
        cs = camera_side(cam, D, a, t)
        det = cs["k1x"] * cs["k2y"] - cs["k1y"] * cs["k2x"]
        cam_ok = det * det > 0
        a32 = np.float32(a)
        r32 = np.sqrt(hx.astype(np.float32) * hx.astype(np.float32) + hy.astype(np.float32) * hy.astype(np.float32) - a32 * a32)
        inside = (np.float32(r_outer) >= r32) & (r32 >= np.float32(r_inner))
        r = np.sqrt(hx * hx + hy * hy - a * a)
        rho2 = hx * hx + hy * hy
        irho = t(1) / np.sqrt(rho2)
        g = (t(1) / r, (r * hx + a * hy) / rho2, (r * hy - a * hx) / rho2)
        u = gas_velocity(g, hx, hy, r, rho2, irho, a, mode, isco, t)
        zero = np.zeros_like(hx)
        vh = (zero, hy * irho, -hx * irho)
        ep = _gunit(g, _axpy(_gdot(g, vh, u), u, vh))
        rh = (zero, hx * irho, hy * irho)
        er = _gunit(g, _axpy(-_gdot(g, rh, ep), ep, _axpy(_gdot(g, rh, u), u, rh)))
        px, py, pz = ph[..., 0], ph[..., 1], ph[..., 2]
        inu = t(1) / (u[0] - (px * u[1] + py * u[2]))
        npr = np.stack([((px * er[1] + py * er[2]) - er[0]) * inu, ((px * ep[1] + py * ep[2]) - ep[0]) * inu, pz * inu], axis=-1)
        n_raw2 = _dot3(npr, npr)                             # 1 for a null k; an interpolated momentum is off the cone
        npr = _unit3(npr)
        b = np.asarray(field, dtype=np.float64)
        b = (b / np.sqrt(np.sum(b * b))).astype(t)           # the host normalizes in binary64 and rounds once
        e = _cross3(npr, np.broadcast_to(b, shape + (3,)))
        s2 = _dot3(e, e)
        eh = e / np.sqrt(np.where(s2 > 0, s2, t(1)))[..., None]
        ft = eh[..., 0] * er[0] + eh[..., 1] * ep[0]
        fv = np.stack([eh[..., 0] * er[1] + eh[..., 1] * ep[1], eh[..., 0] * er[2] + eh[..., 1] * ep[2], eh[..., 2]], axis=-1)
        fU = g[0] * (t(1) + (g[1] * px + g[2] * py))
        kt = t(1) + fU
        kv = np.stack([px - fU * g[1], py - fU * g[2], pz], axis=-1)
        X = np.stack([hx, hy, zero], axis=-1)
        k1, k2 = kappa(X, kt, kv, ft, fv, a)
        x = k1 * cs["k2y"] - cs["k1y"] * k2
        y = cs["k1x"] * k2 - k1 * cs["k2x"]
        den = x * x + y * y
        ok = inside & cam_ok & (s2 > 0) & (den > 0)
        dsafe = np.where(den > 0, den, t(1))
        p = t(fraction) * s2
        aq = np.where(ok, p * ((x * x - y * y) / dsafe), t(0))
        bu = np.where(ok, p * ((t(2) * x * y) / dsafe), t(0))
    if details:
        return aq, bu, ok, dict(alpha=x, beta=y, det=det, s2=s2, ft=ft, fv=fv, kt=kt, kv=kv, k1=k1, k2=k2, u=u, er=er, ep=ep, n=npr, n_raw2=n_raw2, eh=eh,
                                inside=inside, cam=cs, a=a)
    return aq, bu, ok


def frame_stokes(cam, hits, mom, A, mode, field, fraction, r_inner, r_outer, dtype=np.float64):
    """Per record of a Kerr map's HITS (K, H, W, 5) and MOMENTUM (K, H, W, 3) planes: (aq, bu, ok), each (K, H, W).  ``cam`` a
    kerr_ref.build_camera dict."""
    D = K.pixel_rays(cam, dtype)
    hits, mom = np.asarray(hits), np.asarray(mom)
    return crossing_stokes(cam, D[None], hits[..., 0], hits[..., 1], mom, A, mode, field, fraction, r_inner, r_outer, dtype)


# ---- the independent check of the transport rule ------------------------------------------------------------------------------

def metric(x, a):
    """The 4 x 4 covariant metric eta + f l l at the points x (..., 3); ``a`` broadcasts against x[..., 0]."""
    a = np.asarray(a, dtype=np.float64)
    X, Y, Z = x[..., 0], x[..., 1], x[..., 2]
    a2 = a * a
    w = (X * X + Y * Y + Z * Z) - a2
    S = np.sqrt(w * w + 4.0 * a2 * (Z * Z))
    r2 = 0.5 * (w + S)
    r = np.sqrt(r2)
    f = r / S
    Q = r2 + a2
    l = np.stack([np.ones_like(r), (r * X + a * Y) / Q, (r * Y - a * X) / Q, Z / r], axis=-1)
    g = f[..., None, None] * (l[..., :, None] * l[..., None, :])
    g = g + np.diag([-1.0, 1.0, 1.0, 1.0])
    return g


def christoffel(x, a, d=1e-3):
    """Gamma^mu_ab at x (n, 3) from five-point central differences of ``metric`` with spacing d (the metric is stationary)."""
    n = x.shape[0]
    dg = np.zeros((n, 4, 4, 4))                     # dg[n, c, a, b] = d_c g_ab
    a = np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))
    # the centre and, per axis, the offsets +d, -d, +2d, -2d: one evaluation of the metric at 13 points per ray
    off = np.zeros((13, 3))
    for c in range(3):
        off[1 + 4 * c: 5 + 4 * c, c] = (d, -d, 2 * d, -2 * d)
    g = metric(x[:, None, :] + off[None], a[:, None])
    for c in range(3):
        gp, gm, gpp, gmm = (g[:, 1 + 4 * c + k] for k in range(4))
        dg[:, c + 1] = (8.0 * (gp - gm) - (gpp - gmm)) / (12.0 * d)
    ginv = np.linalg.inv(g[:, 0])
    # Gamma^m_ab = 1/2 g^mn (d_a g_nb + d_b g_na - d_n g_ab)
    t1 = np.einsum("xanb->xnab", dg)
    t2 = np.einsum("xbna->xnab", dg)
    return 0.5 * np.einsum("xmn,xnab->xmab", ginv, t1 + t2 - dg)


def _rhs(x, p, f4, a):
    v, dp = K_rhs(x, p, a)
    kt, _ = photon_up_each(x, p, a)
    k4 = np.concatenate([kt[:, None], v], axis=1)
    G = christoffel(x, a)
    return v, dp, -np.einsum("xmab,xa,xb->xm", G, k4, f4)


def K_rhs(x, p, a):
    """kerr_ref.rhs with a spin per ray (its formulas broadcast over an array a)."""
    return K.rhs(x, p, np.broadcast_to(np.asarray(a, dtype=np.float64), (x.shape[0],)))


def photon_up_each(x, p, a):
    """photon_up with a spin per ray."""
    return photon_up(x, p, np.broadcast_to(np.asarray(a, dtype=np.float64), (x.shape[0],)))


def transport(x0, p0, f0, a, lam, h=0.01, watch=None):
    """n photons from x0 (n, 3) with covariant momenta p0 (n, 3), each carrying the contravariant 4-vector f0 (n, 4), spin
    parameter a (n,) each, integrated by RK4 over the affine length lam (n,) in ceil(max(lam) / h) steps of lam / steps each.
    -> (x, p, f) at the end.  ``watch``: a function (x, p, f) -> (n, m) evaluated at the start and after every step; then also
    returned is max |watch - watch at the start| over the steps, (n, m)."""
    x, p, f4 = (np.array(v, dtype=np.float64) for v in (x0, p0, f0))
    a = np.broadcast_to(np.asarray(a, dtype=np.float64), (x.shape[0],))
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (x.shape[0],))
    steps = int(np.ceil(float(lam.max()) / h))
    hh = (lam / steps)[:, None]
    w0 = watch(x, p, f4) if watch else None
    drift = np.zeros_like(w0) if watch else None
    for _ in range(steps):
        v1, a1, b1 = _rhs(x, p, f4, a)
        v2, a2, b2 = _rhs(x + 0.5 * hh * v1, p + 0.5 * hh * a1, f4 + 0.5 * hh * b1, a)
        v3, a3, b3 = _rhs(x + 0.5 * hh * v2, p + 0.5 * hh * a2, f4 + 0.5 * hh * b2, a)
        v4, a4, b4 = _rhs(x + hh * v3, p + hh * a3, f4 + hh * b3, a)
        x = x + hh * (v1 + 2 * v2 + 2 * v3 + v4) / 6.0
        p = p + hh * (a1 + 2 * a2 + 2 * a3 + a4) / 6.0
        f4 = f4 + hh * (b1 + 2 * b2 + 2 * b3 + b4) / 6.0
        if watch:
            drift = np.maximum(drift, np.abs(watch(x, p, f4) - w0))
    return (x, p, f4, drift) if watch else (x, p, f4)


def geodesic_events(x0, d, A, stop_r=None, crossing=None, h=0.01, max_steps=20000):
    """One photon from x0 along d around a hole of spin A by fixed-step RK4 (kerr_ref.rk4_step): -> dict(lam: the affine
    length at the event, r_min: the smallest Kerr-Schild radius seen up to it).  The event: with ``stop_r`` the ray is back
    out at that radius; with ``crossing`` = k it passes z = 0 for the k-th time (1-based), located by bisection on the size
    of the last step."""
    a = float(A) * K.M
    x = np.asarray(x0, dtype=np.float64)[None].copy()
    p = K.initial_momentum(x, np.asarray(d, dtype=np.float64)[None], a)
    hs = np.array([h])
    lam, r_min, seen, turned = 0.0, float(K.ks_radius(x, a)[0]), 0, False
    for _ in range(max_steps):
        nx, npm, _ = K.rk4_step(x, p, hs, a)
        rn = float(K.ks_radius(nx, a)[0])
        if crossing is not None and x[0, 2] * nx[0, 2] < 0:
            seen += 1
            if seen == crossing:
                lo, hi = 0.0, h
                for _ in range(60):
                    mid = 0.5 * (lo + hi)
                    mx, _, _ = K.rk4_step(x, p, np.array([mid]), a)
                    if x[0, 2] * mx[0, 2] < 0:
                        hi = mid
                    else:
                        lo = mid
                return dict(lam=lam + 0.5 * (lo + hi), r_min=min(r_min, rn))
        turned = turned or rn > r_min + 1e-9 and rn > float(K.ks_radius(x, a)[0])
        r_min = min(r_min, rn)
        x, p, lam = nx, npm, lam + h
        if stop_r is not None and turned and rn >= stop_r:
            return dict(lam=lam, r_min=r_min)
        if rn < K.r_plus(float(A)) * 1.001:
            raise AssertionError("the ray fell into the hole")
    raise AssertionError("no event on the ray")


# ---- records without a device ----------------------------------------------------------------------------------------------------

def march_records(cam, A, h_base=0.1, r_inner=2.0, r_outer=15.0, slots=4, dtype=np.float64):
    """kerr_ref's march of every pixel's ray of a kerr_ref.build_camera dict keeping, per crossing of the annulus, the hit
    point and the photon's momentum interpolated to it as the device's build does: (hits (slots, H, W, 5), mom (slots, H, W,
    3), crossings (H, W)).  hits[..., 2:5] = -dx/dl at the start of the crossing's step (the model redshift's to_cam)."""
    t = np.dtype(dtype).type
    a = t(A) * t(K.M)
    D = K.pixel_rays(cam, dtype).reshape(-1, 3)
    n = D.shape[0]
    x = np.broadcast_to(cam["pos"].astype(dtype), (n, 3)).copy()
    p = K.initial_momentum(x, D, a)
    rp = t(K.r_plus(float(A)))
    r_esc, hb = t(cam["r_escape"]), t(h_base)
    max_iter = int(np.float32(cam["r_escape"]) * np.float32(40.0) / np.float32(h_base))
    max_affine = t(np.float32(cam["r_escape"]) * np.float32(40.0))
    r = K.ks_radius(x, a)
    affine = np.zeros(n, dtype=dtype)
    idx = np.arange(n)
    hits, mom = np.zeros((slots, n, 5)), np.zeros((slots, n, 3))
    count = np.zeros(n, dtype=np.int32)
    it = 0
    while idx.size and it < max_iter:
        h = hb * K.dt_fac(r)
        nx, npm, v1 = K.rk4_step(x, p, h, a)
        rn = K.ks_radius(nx, a)
        aff = affine + h
        ended = (rn < rp) | (rn > r_esc) | (aff > max_affine)
        z0, z1 = x[:, 2], nx[:, 2]
        c = np.nonzero((z0 * z1 < 0) & ~ended)[0]
        if c.size:
            tf = z0[c] / (z0[c] - z1[c] + t(1e-8))
            hx = x[c, 0] + tf * (nx[c, 0] - x[c, 0])
            hy = x[c, 1] + tf * (nx[c, 1] - x[c, 1])
            hr = np.sqrt(hx * hx + hy * hy - a * a)
            ok = (t(r_outer) >= hr) & (hr >= t(r_inner))
            c, tf, hx, hy = c[ok], tf[ok], hx[ok], hy[ok]
            ray = idx[c]
            keep = count[ray] < slots
            rk, ck = ray[keep], c[keep]
            hits[count[rk], rk, 0], hits[count[rk], rk, 1] = hx[keep], hy[keep]
            hits[count[rk], rk, 2:5] = -v1[ck]
            mom[count[rk], rk] = p[ck] + tf[keep, None] * (npm[ck] - p[ck])
            count[ray] += 1
        it += 1
        go = ~ended
        idx, x, p, r, affine = idx[go], nx[go], npm[go], rn[go], aff[go]
    H, W = cam["height"], cam["width"]
    return hits.reshape(slots, H, W, 5), mom.reshape(slots, H, W, 3), count.reshape(H, W)
