"""CPU reference of the point stars (include/bhr.h "point stars"; DESIGN.md 4 "Point stars"), in NumPy.

Imports nothing from the product.  Brute force: every star against every used triangle -- no grid of bins.  binary64 by default;
dtype=np.float32 evaluates every operation of the model in f32 (the float32 switch).

The model, restated.  A star: unit direction u, RGB flux Phi (sky value x steradian).  Cell (i, j), 0 <= i < W - 1,
0 <= j < H - 1, has the pixel centres P00 = (i, j), P10 = (i+1, j), P01 = (i, j+1), P11 = (i+1, j+1) and is cut into
T0 = (P00, P10, P01) and T1 = (P11, P01, P10).  For a triangle (a, b, c): e_* the escape directions, n_* the camera-side pixel
directions.  USED: all three status 1 and min(e_a.e_b, e_b.e_c, e_c.e_a) >= cos(max_span).
  Omega(a, b, c) = 2 atan2(|a . ((b - a) x (c - a))|, 1 + a.b + b.c + c.a)
  s_c = u . (e_a x e_b), s_a = u . (e_b x e_c), s_b = u . (e_c x e_a)  [as u . ((e_a - u) x (e_b - u)) ...: the same determinants]
  inside: all >= 0 or all <= 0, and u . (e_a + e_b + e_c) > 0;  w_x = s_x / (s_a + s_b + s_c), a zero sum contributes nothing
  D = Phi / (2 Omega_cam) * min(Omega_cam / Omega_sky, max_magnification), spread over the cell's four corner pixels with the
  bilinear weights of the image position sum_x w_x P_x.
A pixel on the map's overflow list gets its star light here like any other; the DEVICE's frame gives it none (the strict fix
kernel stores it) -- the plane S itself has no such exception.
"""
import numpy as np

DEFAULT_MAX_MAGNIFICATION = 32.0
DEFAULT_MAX_SPAN_DEG = 10.0


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def solid_angle(a, b, c):
    """Van Oosterom and Strackee with the triple product on differences."""
    t = a.dtype.type
    num = np.abs(_dot(a, _cross(b - a, c - a)))
    den = t(1) + _dot(a, b) + _dot(b, c) + _dot(c, a)
    return t(2) * np.arctan2(num, den)


def turn_z(v, angle):
    """v (..., 3) turned about z by `angle` radians, in binary64."""
    v = np.asarray(v, dtype=np.float64)
    c, s = np.cos(angle), np.sin(angle)
    return np.stack([c * v[..., 0] - s * v[..., 1], s * v[..., 0] + c * v[..., 1], v[..., 2]], axis=-1)


def triangles(status, esc, ncam, max_span_deg=DEFAULT_MAX_SPAN_DEG, dtype=np.float64):
    """Every triangle of three escaped rays: dict of flat arrays -- cell (n, 2) = (i, j), second (n,) bool (T1), e (n, 3, 3) and
    n (n, 3, 3) corner directions in the order a, b, c, used (n,) bool (the span rule), o_sky, o_cam, mag."""
    t = np.dtype(dtype).type
    status = np.asarray(status)
    H, W = status.shape
    esc = np.asarray(esc, dtype=dtype)
    ncam = np.asarray(ncam, dtype=dtype)
    jj, ii = np.meshgrid(np.arange(H - 1), np.arange(W - 1), indexing="ij")
    jj, ii = jj.ravel(), ii.ravel()
    out = []
    for second in (False, True):
        if not second:
            ca, cb, cc = (jj, ii), (jj, ii + 1), (jj + 1, ii)
        else:
            ca, cb, cc = (jj + 1, ii + 1), (jj + 1, ii), (jj, ii + 1)
        ok = (status[ca] == 1) & (status[cb] == 1) & (status[cc] == 1)
        e = np.stack([esc[ca][ok], esc[cb][ok], esc[cc][ok]], axis=1)
        n = np.stack([ncam[ca][ok], ncam[cb][ok], ncam[cc][ok]], axis=1)
        out.append((np.stack([ii[ok], jj[ok]], axis=-1), np.full(int(ok.sum()), second), e, n))
    cell = np.concatenate([o[0] for o in out])
    second = np.concatenate([o[1] for o in out])
    e = np.concatenate([o[2] for o in out])
    n = np.concatenate([o[3] for o in out])
    span = np.minimum(np.minimum(_dot(e[:, 0], e[:, 1]), _dot(e[:, 1], e[:, 2])), _dot(e[:, 2], e[:, 0]))
    used = span >= t(np.cos(np.radians(float(max_span_deg))))
    with np.errstate(divide="ignore", invalid="ignore"):
        o_sky = solid_angle(e[:, 0], e[:, 1], e[:, 2])
        o_cam = solid_angle(n[:, 0], n[:, 1], n[:, 2])
        mag = o_cam / o_sky
    return dict(cell=cell, second=second, e=e, n=n, used=used, o_sky=o_sky, o_cam=o_cam, mag=mag)


def star_plane(status, esc, ncam, dirs, flux, max_magnification=DEFAULT_MAX_MAGNIFICATION, max_span_deg=DEFAULT_MAX_SPAN_DEG,
               dtype=np.float64, prefilter=True, details=False):
    """The star plane S (H, W, 3) in `dtype`: status (H, W) fates, esc (H, W, 3) escape directions (already turned for a turned
    view), ncam (H, W, 3) camera-side pixel directions, dirs (n, 3) unit star directions, flux (n, 3).

    prefilter: pairs (triangle, star) are first thinned, always in binary64, by one matrix product -- a star inside a used
    triangle lies within the triangle's largest vertex angle (+ 1e-3 rad) of its normalized vertex sum; every pair that passes
    gets the full test.  prefilter=False tests every pair (the same plane; slow).
    details: also a dict with images, capped, skipped_span, the triangles() dict as tri, and the pairs' (tri index, star index,
    fx, fy, magnification used)."""
    t = np.dtype(dtype).type
    H, W = np.asarray(status).shape
    tri = triangles(status, esc, ncam, max_span_deg, dtype)
    u_all = np.asarray(dirs, dtype=dtype)
    phi_all = np.asarray(flux, dtype=dtype)
    S = np.zeros((H, W, 3), dtype=dtype)
    used = np.nonzero(tri["used"])[0]
    stats = dict(images=0, capped=int((tri["mag"][used] > t(max_magnification)).sum()), skipped_span=int((~tri["used"]).sum()), tri=tri)
    pairs_out = []
    if len(u_all) and len(used):
        u64 = np.asarray(dirs, dtype=np.float64)
        for lo in range(0, len(used), 1024):
            ti = used[lo:lo + 1024]
            if prefilter:
                e64 = tri["e"][ti].astype(np.float64)
                m = e64.sum(axis=1)
                m /= np.linalg.norm(m, axis=-1, keepdims=True)
                cos_r = np.min(np.einsum("tk,tvk->tv", m, e64), axis=1)
                lim = np.cos(np.arccos(np.clip(cos_r, -1.0, 1.0)) + 1e-3)
                tk, sk = np.nonzero((m @ u64.T) >= lim[:, None])
            else:
                tk, sk = np.nonzero(np.ones((len(ti), len(u_all)), dtype=bool))
            if not len(tk):
                continue
            tg = ti[tk]
            u = u_all[sk]
            ea, eb, ec = tri["e"][tg, 0], tri["e"][tg, 1], tri["e"][tg, 2]
            da, db, dc = ea - u, eb - u, ec - u
            sc, sa, sb = _dot(u, _cross(da, db)), _dot(u, _cross(db, dc)), _dot(u, _cross(dc, da))
            front = _dot(u, (ea + eb) + ec) > 0
            inside = (((sa >= 0) & (sb >= 0) & (sc >= 0)) | ((sa <= 0) & (sb <= 0) & (sc <= 0))) & front
            tot = (sa + sb) + sc
            inside &= tot != 0
            tg, sk, sa, sb, sc, tot = tg[inside], sk[inside], sa[inside], sb[inside], sc[inside], tot[inside]
            if not len(tg):
                continue
            wa, wb, wc = sa / tot, sb / tot, sc / tot
            second = tri["second"][tg]
            fx = np.where(second, wa + wc, wb)
            fy = np.where(second, wa + wb, wc)
            magc = np.minimum(tri["mag"][tg], t(max_magnification))
            q = magc / (t(2) * tri["o_cam"][tg])
            d = phi_all[sk] * q[:, None]
            i, j = tri["cell"][tg, 0], tri["cell"][tg, 1]
            one = t(1)
            np.add.at(S, (j, i), d * ((one - fx) * (one - fy))[:, None])
            np.add.at(S, (j, i + 1), d * (fx * (one - fy))[:, None])
            np.add.at(S, (j + 1, i), d * ((one - fx) * fy)[:, None])
            np.add.at(S, (j + 1, i + 1), d * (fx * fy)[:, None])
            stats["images"] += len(tg)
            if details:
                pairs_out.append(np.column_stack([tg, sk, fx, fy, magc]))
    if details:
        stats["pairs"] = np.concatenate(pairs_out) if pairs_out else np.zeros((0, 5))
        return S, stats
    return S


def distance(a, b):
    """The distance of two planes the tests' bar is put on: per channel the 99.5th percentile of |a - b| over the pixels, the
    largest of the three, as a share of the largest value of b.  (A star within rounding of a triangle's edge can be inside in
    one evaluation and outside in the other: single pixels then differ by a whole deposit.  The tests bound the SHARE of such
    pixels separately -- 0.5 % beyond 1e-3 of the maximum -- so the distance leaves that share out.)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    peak = float(b.max())
    if peak <= 0:
        return float(np.abs(a - b).max())
    return max(float(np.percentile(np.abs(a[..., c] - b[..., c]), 99.5)) for c in range(3)) / peak


def outlier_share(a, b, rel=1e-3):
    """Share of the pixels where any channel of a and b differs by more than rel of b's largest value."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    peak = float(b.max())
    return float((np.abs(a - b).max(axis=-1) > rel * peak).mean())
