"""CPU reference of the polarisation (include/bhr.h "polarisation"; no test functions).

Three independent pieces:
  * ``crossing_stokes``: the model's steps for arrays of crossings in NumPy, dtype float64 or float32 (every operation then
    rounds to f32, as the kernel's does);
  * ``transport``: a binary64 RK4 integrator of the photon geodesic and the parallel transport df/dl = -Gamma k f in
    Schwarzschild coordinates, which knows nothing of the planar rule the model uses;
  * ``march_records``: a plain binary64 march of a view's rays (d2x/dl2 = -1.5 L^2 x / r^5, fixed step) that finds disk
    crossings and the photon's direction there -- records like the ray map's, made without a device, for measuring how far the
    f32 evaluation of the model is from the f64 one.
Units r_s = 1, F(r) = 1 - 1 / r.
"""
import numpy as np

LUMA = (0.2126, 0.7152, 0.0722)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _scale(s, v):
    return s[..., None] * v


def _unit(v):
    return _scale(1 / np.sqrt(_dot(v, v)), v)


def camera_dict(cam):
    """The f32 camera a renderer uploads (a ctypes bhr_camera) as float64 arrays of those f32 values."""
    return {"pos": np.array(list(cam.pos), dtype=np.float64), "right": np.array(list(cam.right), dtype=np.float64),
            "up": np.array(list(cam.up), dtype=np.float64), "forward": np.array(list(cam.forward), dtype=np.float64),
            "pw": float(cam.pixel_width), "ph": float(cam.pixel_height)}


def pixel_dirs(cam, width, height, dtype=np.float64):
    """(H, W, 3) unit launch directions D of the pixels' rays, the march's pixel_ray operation by operation in ``dtype``."""
    t = dtype
    cp, cr, cu, cf = (np.asarray(cam[k], dtype=t) for k in ("pos", "right", "up", "forward"))
    pw, ph = t(cam["pw"]), t(cam["ph"])
    center = cp + t(1) * cf
    half_w = pw * t(width) / t(2)
    half_h = ph * t(height) / t(2)
    tl = (center - half_w * cr) + half_h * cu
    px = (np.arange(width, dtype=t) + t(0.5)) * pw
    py = (np.arange(height, dtype=t) + t(0.5)) * ph
    pos = (tl[None, None, :] + px[None, :, None] * cr[None, None, :]) - py[:, None, None] * cu[None, None, :]
    return _unit(pos - cp[None, None, :]).astype(t)


def crossing_stokes(cam, D, hx, hy, w, tilt_deg, field, fraction, r_inner, r_outer, dtype=np.float64, details=False):
    """The model per crossing.  ``D`` (..., 3) launch directions, ``hx``, ``hy`` (...) hit point, ``w`` (..., 3) to_cam, all
    broadcastable to one shape.  -> (a, b, ok): a = p cos 2chi, b = p sin 2chi (0 where not ok), ok = the crossing lies in the
    annulus (the device's own f32 test), its ray is not radial and s2 > 0.  ``details``: also a dict of intermediates."""
    t = dtype
    C = np.asarray(cam["pos"], dtype=t)
    R, U = np.asarray(cam["right"], dtype=t), np.asarray(cam["up"], dtype=t)
    D = np.asarray(D, dtype=t)
    hx, hy = np.asarray(hx, dtype=t), np.asarray(hy, dtype=t)
    w = np.asarray(w, dtype=t)
    shape = np.broadcast_shapes(D.shape[:-1], hx.shape, w.shape[:-1])
    D = np.broadcast_to(D, shape + (3,))
    hx, hy = np.broadcast_to(hx, shape), np.broadcast_to(hy, shape)
    w = np.broadcast_to(w, shape + (3,))
    # the tilt as the march has it: f32 radians, f32 tan / sin / cos
    tilt = np.float32(tilt_deg) * np.float32(3.14159274101257324) / np.float32(180.0)
    tan_t, sin_t, cos_t = (t(np.float32(f(tilt))) for f in (np.tan, np.sin, np.cos))
    with np.errstate(all="ignore"):
        # 1. the plane's normal
        CxD = _cross(np.broadcast_to(C, shape + (3,)), D)
        cxd = np.sqrt(_dot(CxD, CxD))
        radial = cxd < t(1e-6) * np.sqrt(_dot(C, C))
        N = _scale(1 / np.where(radial, t(1), cxd), CxD)
        # the device's annulus test, in f32 whatever dtype: it decides which crossings exist
        hr32 = np.sqrt(hx.astype(np.float32) * hx.astype(np.float32) + hy.astype(np.float32) * hy.astype(np.float32))
        inside = (np.float32(r_outer) >= hr32) & (hr32 >= np.float32(r_inner))
        # 2. emission point and direction
        P = np.stack([hx, hy, hy * tan_t], axis=-1)
        r_em = np.sqrt(_dot(P, P))
        rh = _scale(1 / r_em, P)
        r = np.maximum(r_em, t(1) + t(1e-3))
        sF = np.sqrt(t(1) - t(1) / r)
        wr = _dot(w, rh)
        K = _scale(wr / sF, rh) + (w - _scale(wr, rh))
        K = _unit(K - _scale(_dot(K, N), N))
        # 3. the gas
        dn = np.broadcast_to(np.array([0, -sin_t, cos_t], dtype=t), shape + (3,))
        vh = _cross(rh, dn)
        vn = np.sqrt(_dot(vh, vh))
        fallback = np.broadcast_to(np.array([0, 1, 0], dtype=t), shape + (3,))
        vh = np.where((vn > t(1e-6))[..., None], vh / np.where(vn > t(1e-6), vn, t(1))[..., None], fallback)
        omega = np.sqrt(t(0.5) / (r * r * r))
        beta = np.minimum(r * omega / sF, t(0.99))
        gamma = t(1) / np.sqrt(t(1) - beta * beta)
        # 4. the photon in the gas frame
        kv = _dot(K, vh)
        inv = t(1) / (gamma * (t(1) - beta * kv))
        npr = _scale(inv, K + _scale((gamma - t(1)) * kv - gamma * beta, vh))
        # 5. the field
        b = np.asarray(field, dtype=np.float64)
        b = (b / np.sqrt(np.sum(b * b))).astype(t)           # the host normalizes in binary64 and rounds once
        B = _unit((b[0] * rh + b[1] * vh) + b[2] * dn)
        e = _cross(npr, B)
        s2 = _dot(e, e)
        eh = _scale(1 / np.sqrt(np.where(s2 > 0, s2, t(1))), e)
        # 6. back to the static frame
        ev = _dot(eh, vh)
        f = (eh + _scale((gamma - t(1)) * ev, vh)) - _scale(gamma * beta * ev, K)
        # 7. the conserved angle
        cpsi, spsi = _dot(f, N), _dot(f, _cross(N, K))
        # 8. at the camera
        Rb = np.broadcast_to(R, shape + (3,))
        ex = _unit(Rb - _scale(_dot(Rb, D), D))
        ey = _cross(D, ex)
        ey = np.where((_dot(ey, np.broadcast_to(U, shape + (3,))) < 0)[..., None], -ey, ey)
        M = _cross(N, -D)
        x = cpsi * _dot(N, ex) + spsi * _dot(M, ex)
        y = cpsi * _dot(N, ey) + spsi * _dot(M, ey)
        den = x * x + y * y
        ok = inside & ~radial & (s2 > 0) & (den > 0)
        dsafe = np.where(den > 0, den, t(1))
        p = t(fraction) * s2
        a = np.where(ok, p * ((x * x - y * y) / dsafe), t(0))
        bq = np.where(ok, p * ((t(2) * x * y) / dsafe), t(0))
    if details:
        return a, bq, ok, {"f": f, "K": K, "N": N, "s2": s2, "cpsi": cpsi, "spsi": spsi, "inside": inside, "radial": radial}
    return a, bq, ok


def frame_stokes(cam, width, height, hits, tilt_deg, field, fraction, r_inner, r_outer, dtype=np.float64):
    """Per record of a ray map's HITS plane (K, H, W, 5 | 9): (a, b, ok), each (K, H, W)."""
    D = pixel_dirs(cam, width, height, dtype)
    hits = np.asarray(hits)
    return crossing_stokes(cam, D[None], hits[..., 0], hits[..., 1], hits[..., 2:5], tilt_deg, field, fraction, r_inner, r_outer, dtype)


# ---- the independent check of the transport rule ------------------------------------------------------------------------------

def _rhs(y):
    """d/dl of (x, k, f) in Schwarzschild coordinates (t, r, theta, phi): the geodesic and df/dl = -Gamma k f."""
    r, th = y[1], y[2]
    k, f = y[4:8], y[8:12]
    F = 1.0 - 1.0 / r
    s, c = np.sin(th), np.cos(th)
    g_ttr = 1.0 / (2.0 * r * r * F)
    g_rtt = F / (2.0 * r * r)
    g_rrr = -1.0 / (2.0 * r * r * F)
    g_rthth = -r * F
    g_rphph = -r * F * s * s
    g_thrth = 1.0 / r
    g_thphph = -s * c
    g_phrph = 1.0 / r
    g_phthph = c / s

    def contract(a, b):
        return np.array([g_ttr * (a[0] * b[1] + a[1] * b[0]),
                         g_rtt * a[0] * b[0] + g_rrr * a[1] * b[1] + g_rthth * a[2] * b[2] + g_rphph * a[3] * b[3],
                         g_thrth * (a[1] * b[2] + a[2] * b[1]) + g_thphph * a[3] * b[3],
                         g_phrph * (a[1] * b[3] + a[3] * b[1]) + g_phthph * (a[2] * b[3] + a[3] * b[2])])
    return np.concatenate([k, -contract(k, k), -contract(k, f)])


def _frame(x):
    """The static observer's spatial triad at coordinates x as Cartesian unit vectors (r_hat, theta_hat, phi_hat)."""
    th, ph = x[2], x[3]
    st, ct, sp, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
    return np.array([st * cp, st * sp, ct]), np.array([ct * cp, ct * sp, -st]), np.array([-sp, cp, 0.0])


def _to_static(x, v):
    """Coordinate components v^mu at x -> (time component, Cartesian 3-vector) in the static observer's orthonormal frame."""
    r, th = x[1], x[2]
    F = 1.0 - 1.0 / r
    er, eth, eph = _frame(x)
    return np.sqrt(F) * v[0], (v[1] / np.sqrt(F)) * er + (r * v[2]) * eth + (r * np.sin(th) * v[3]) * eph


def psi_of(f, N, K):
    """Step 7: (cos psi, sin psi) of a unit vector f perpendicular to K."""
    return float(np.dot(f, N)), float(np.dot(f, np.cross(N, K)))


def transport(r_peri, plane_normal, psi0, r_start=20.0, r_end=25.0, h=0.01):
    """A photon launched inwards at r_start in the plane with unit normal ``plane_normal``, periapsis ``r_peri``, carrying the
    unit polarisation vector cos psi0 N + sin psi0 (N x K); integrated by RK4 with step h until it is back out at r_end.
    -> dict(psi_start, psi_end, swept: the angle between the start and end positions' directions accumulated along the ray,
    N_drift: how far the plane's normal formed from the end state is from the start's)."""
    n = np.asarray(plane_normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    e1 = np.cross(n, [0.0, 0.0, 1.0])
    e1 = e1 / np.linalg.norm(e1) if np.linalg.norm(e1) > 1e-9 else np.array([1.0, 0.0, 0.0])
    e2 = np.cross(n, e1)
    pos = r_start * e1
    b = r_peri / np.sqrt(1.0 - 1.0 / r_peri)
    F0 = 1.0 - 1.0 / r_start
    sin_a = b * np.sqrt(F0) / r_start
    K = -np.sqrt(1.0 - sin_a * sin_a) * e1 + sin_a * e2
    N = np.cross(pos, K)
    N = N / np.linalg.norm(N)
    f3 = np.cos(psi0) * N + np.sin(psi0) * np.cross(N, K)
    x = np.array([0.0, r_start, np.arccos(pos[2] / r_start), np.arctan2(pos[1], pos[0])])
    er, eth, eph = _frame(x)

    def to_coord(tc, v):
        return np.array([tc / np.sqrt(F0), np.sqrt(F0) * np.dot(v, er), np.dot(v, eth) / r_start, np.dot(v, eph) / (r_start * np.sin(x[2]))])
    y = np.concatenate([x, to_coord(1.0, K), to_coord(0.0, f3)])
    swept, prev = 0.0, pos / r_start
    turned = False
    for _ in range(int(200.0 / h)):
        k1 = _rhs(y)
        k2 = _rhs(y + 0.5 * h * k1)
        k3 = _rhs(y + 0.5 * h * k2)
        k4 = _rhs(y + h * k3)
        y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        cur = _frame(y[0:4])[0]
        swept += float(np.arccos(np.clip(np.dot(cur, prev), -1.0, 1.0)))
        prev = cur
        turned = turned or y[5] > 0.0
        if turned and y[1] >= r_end:
            break
    else:
        raise AssertionError("the ray did not come back out")
    kt, K1 = _to_static(y[0:4], y[4:8])
    K1 = K1 / kt                                   # a null vector: |spatial part| = time component
    ft, f1 = _to_static(y[0:4], y[8:12])
    f1 = f1 - ft * K1                              # the gauge f -> f + c k that takes the time component away
    f1 = f1 / np.linalg.norm(f1)
    N1 = np.cross(y[1] * _frame(y[0:4])[0], K1)
    N1 = N1 / np.linalg.norm(N1)
    c0, s0 = psi_of(f3, N, K)
    c1, s1 = psi_of(f1, N, K1)
    return {"psi_start": float(np.arctan2(s0, c0)), "psi_end": float(np.arctan2(s1, c1)), "swept": swept,
            "N_drift": float(np.linalg.norm(N1 - N)), "r_min_seen": float(y[1])}


# ---- records without a device ----------------------------------------------------------------------------------------------------

def march_records(cam, width, height, tilt_deg, r_inner, r_outer, r_escape, h=0.05, slots=4):
    """A plain binary64 march of every pixel's ray: (hits (slots, H, W, 5), crossings (H, W)) in the ray map's record format --
    hit_x, hit_y of each crossing of the tilted disk plane inside the annulus and to_cam = -direction at the start of the
    crossing step.  A fixed-step RK4 of d2x/dl2 = -1.5 L^2 x / r^5; close to the device's records, not equal to them."""
    D = pixel_dirs(cam, width, height).reshape(-1, 3)
    n = D.shape[0]
    p = np.broadcast_to(np.asarray(cam["pos"], dtype=np.float64), (n, 3)).copy()
    d = D.copy()
    tan_t = np.tan(np.radians(tilt_deg))
    L2 = np.sum(np.cross(d, p) ** 2, axis=1)
    hits = np.zeros((slots, n, 5))
    count = np.zeros(n, dtype=np.int32)
    alive = np.ones(n, dtype=bool)

    def acc(s):
        r2 = np.sum(s * s, axis=1)
        return (-1.5 * L2 / (r2 * r2 * np.sqrt(r2)))[:, None] * s
    for _ in range(int(40.0 * r_escape / h)):
        if not alive.any():
            break
        k1p, k1d = h * d, h * acc(p)
        k2p, k2d = h * (d + 0.5 * k1d), h * acc(p + 0.5 * k1p)
        k3p, k3d = h * (d + 0.5 * k2d), h * acc(p + 0.5 * k2p)
        k4p, k4d = h * (d + k3d), h * acc(p + k3p)
        pn = p + (k1p + 2 * k2p + 2 * k3p + k4p) / 6.0
        dn = d + (k1d + 2 * k2d + 2 * k3d + k4d) / 6.0
        f0, f1 = p[:, 2] - p[:, 1] * tan_t, pn[:, 2] - pn[:, 1] * tan_t
        cross = alive & (f0 * f1 < 0)
        if cross.any():
            tt = f0 / np.where(cross, f0 - f1, 1.0)
            hp = p + tt[:, None] * (pn - p)
            hr = np.hypot(hp[:, 0], hp[:, 1])
            take = cross & (hr >= r_inner) & (hr <= r_outer)
            idx = np.nonzero(take & (count < slots))[0]
            hits[count[idx], idx, 0] = hp[idx, 0]
            hits[count[idx], idx, 1] = hp[idx, 1]
            hits[count[idx], idx, 2:5] = -d[idx]
            count[take] += 1
        r2 = np.sum(pn * pn, axis=1)
        alive = alive & (r2 > 1.0) & (r2 < r_escape * r_escape)
        p = np.where(alive[:, None], pn, p)
        d = np.where(alive[:, None], dn, d)
    return hits.reshape(slots, height, width, 5), count.reshape(height, width)
