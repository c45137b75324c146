"""The Kerr polarisation's model on the CPU (tests/kerr_polar_ref.py; include/bhr.h "Kerr polarisation"): the Walker-Penrose
constant in the march's Kerr-Schild chart against a parallel transport that knows nothing of it, the model end to end, its
mirror symmetry, the hole that does not spin against the Schwarzschild pass's model, and the float32 evaluation's distance from
the binary64 one, which sets the device's bar (tests/test_gpu_kerr_polarization.py).

Measured here (binary64, fov 90, r_disk 2 .. 15, step 0.1 -- the GPU test's scene):
  conservation, h = 0.01, camera (6, 0, 0.5) out to r = 14, periapsis 1.82 / 2.24 / 2.83 at A = 0.9 / -0.6 / 0.9:
      |d kappa1| <= 9.1e-11, |d kappa2| <= 2.1e-11; with the other sign of a the same rays drift by 0.030 .. 0.72
  end to end (h = 0.02): the transported camera vector against f_em in the gas frame, <= 2.4e-8 rad over the nine rays
  float32 against binary64 on the records of the three views, four spins, both modes, four fields, Pi_0 = 1:
      2.07e-6 at 64 x 36, 1.55e-6 at 33 x 9, 2.00e-6 at 9 x 7, 1.22e-6 at 5 x 3           -> F32_DISTANCE = 2.08e-6
  A = 0 (model) against polar_ref.crossing_stokes on the same records, the record's own to_cam for the Schwarzschild model:
      0.097 at (6, 0, 0.5), 0.223 at (2.5, 2, 1.2), 0.159 at (4, 3, 2); 9.0e-3 from (100, 40, 20) at fov 16: the camera stretch
      the Schwarzschild pass ignores, and the ray's bend between the start of the crossing's step, where to_cam is taken, and
      the hit (given the photon at the hit instead: 0.049 / 0.113 / 0.063 and 6.1e-4)        -> SCHWARZSCHILD_DISTANCE = 0.2233
  single-crossing share of the pixels with a crossing: 0.857 .. 0.976 at the three larger sizes, >= 0.80 at 5 x 3"""
import functools

import numpy as np
import pytest

import kerr_polar_ref as P
import kerr_redshift_ref as R
import kerr_ref as K
import polar_ref as S

FOV = 90.0
R_IN, R_OUT = 2.0, 15.0
VIEWS = ((6.0, 0.0, 0.5), (2.5, 2.0, 1.2), (4.0, 3.0, 2.0))
SPINS = (0.0, 0.6, -0.9, 0.998)
FIELDS = ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.8, 0.5))
SIZES = ((64, 36), (33, 9), (9, 7), (5, 3))


def _direction(cam, s, u):
    d = cam["forward"].astype(np.float64) + s * cam["right"].astype(np.float64) + u * cam["up"].astype(np.float64)
    return d / np.linalg.norm(d)


# ---- 1. conservation against the blind transport ------------------------------------------------------------------------------------
# (spin, s of the launch direction normalize(forward + s right + 0.1 up), periapsis in r_s): the three rays of the issue
CONSERVATION_RAYS = ((0.9, 0.40774992209917393, 1.82), (-0.6, 0.6180990942473725, 2.24), (0.9, 0.6438629830579887, 2.83))


def test_walker_penrose_is_conserved_and_the_sign_of_a_is_pinned():
    cam = K.build_camera((6.0, 0.0, 0.5), 60.0, 8, 8)
    n = len(CONSERVATION_RAYS)
    x0 = np.tile(cam["pos"].astype(np.float64), (n, 1))
    a = np.array([A * K.M for A, _, _ in CONSERVATION_RAYS])
    d = np.array([_direction(cam, s, 0.1) for _, s, _ in CONSERVATION_RAYS])
    p0 = np.array([K.initial_momentum(x0[i:i + 1], d[i:i + 1], a[i])[0] for i in range(n)])
    lam = []
    for i, (A, _, peri) in enumerate(CONSERVATION_RAYS):
        ev = P.geodesic_events(x0[i], d[i], A, stop_r=14.0)
        assert abs(ev["r_min"] - peri) < 5e-3, (A, ev)
        lam.append(ev["lam"])
    # a polarisation orthogonal to k: a mix of the lifted image axes
    f0 = []
    for i in range(n):
        cs = P.camera_side(cam, d[i], a[i])
        f0.append(np.concatenate([[0.3 * cs["Ext"] + 0.8 * cs["Eyt"]], 0.3 * cs["ex"] + 0.8 * cs["ey"]]))

    def watch(x, p, f):
        kt, kv = P.photon_up_each(x, p, a)
        right = P.kappa(x, kt, kv, f[:, 0], f[:, 1:], a)
        wrong = P.kappa(x, kt, kv, f[:, 0], f[:, 1:], -a)
        return np.stack(right + wrong, axis=1)
    x, _, _, drift = P.transport(x0, p0, np.array(f0), a, np.array(lam), h=0.01, watch=watch)
    print("final radii", K.ks_radius(x, a), "drift of kappa1, kappa2 and of both with -a:\n", drift)
    assert (np.abs(K.ks_radius(x, a) - 14.0) < 0.05).all()
    assert (drift[:, :2] <= 1e-8).all(), drift
    assert (drift[:, 2:] > 1e-2).all(), drift


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------------
# (spin, mode, camera, s, u of the launch direction, which passage of z = 0): first crossings at the three spins in both modes,
# a plunging-gas hit (A = -0.9, exact, r = 1.98 inside the retrograde ISCO at 4.36) and second crossings
E2E = ((0.6, "model", (6, 0, 0.5), 0.3, -0.35, 1), (0.6, "exact", (6, 0, 0.5), -0.4, -0.3, 1),
       (-0.9, "model", (2.5, 2, 1.2), 0.2, -0.5, 1), (-0.9, "exact", (2.5, 2, 1.2), 0.2, -0.5, 1), (-0.9, "exact", (6, 0, 0.5), 0.15, -0.42, 1),
       (0.998, "model", (4, 3, 2), 0.3, -0.6, 1), (0.998, "exact", (4, 3, 2), -0.2, -0.7, 1),
       (0.6, "exact", (6, 0, 0.5), 0.45, -0.4, 2), (-0.9, "model", (6, 0, 0.5), 0.45, -0.4, 2))


def test_camera_vector_transported_to_the_gas_is_the_emitted_one():
    field, r_in = (0.3, 0.8, 0.5), 1.2
    cams, ds = [], []
    x0, p0, a, lam = [], [], [], []
    for A, mode, pos, s, u, which in E2E:
        cam = K.build_camera(pos, 60.0, 8, 8)
        d = _direction(cam, s, u)
        x = cam["pos"].astype(np.float64)
        a.append(0.5 * float(np.float32(A)))
        lam.append(P.geodesic_events(x, d, float(np.float32(A)), crossing=which)["lam"])
        cams.append(cam)
        ds.append(d)
        x0.append(x)
        p0.append(K.initial_momentum(x[None], d[None], a[-1])[0])
    x0, p0, a, lam = (np.array(v) for v in (x0, p0, a, lam))
    n = len(E2E)
    xe, pe, _ = P.transport(x0, p0, np.zeros((n, 4)), a, lam, h=0.02)     # the geodesic alone: the crossing and the photon there
    assert (np.abs(xe[:, 2]) < 1e-6).all()
    f0, det = [], []
    plunging = second = 0
    for i, (A, mode, pos, s, u, which) in enumerate(E2E):
        aq, bu, ok, dt = P.crossing_stokes(cams[i], ds[i], xe[i, 0], xe[i, 1], pe[i], A, mode, field, 1.0, r_in, R_OUT, details=True)
        assert ok and np.hypot(aq, bu) > 0.05
        r = np.sqrt(xe[i, 0] ** 2 + xe[i, 1] ** 2 - a[i] ** 2)
        plunging += mode == "exact" and r < R.isco_orbit(A)[0]
        second += which == 2
        cs = dt["cam"]
        f0.append(np.concatenate([[dt["alpha"] * cs["Ext"] + dt["beta"] * cs["Eyt"]], dt["alpha"] * cs["ex"] + dt["beta"] * cs["ey"]]))
        det.append(dt)
    assert plunging >= 1 and second >= 2
    _, _, fe = P.transport(x0, p0, np.array(f0), a, lam, h=0.02)
    worst = 0.0
    for i in range(n):
        dt = det[i]
        G = P.metric(xe[i], a[i])
        lift = lambda v: np.array([v[0], v[1], v[2], 0.0])
        u4, er4, ep4, ez4 = lift(dt["u"]), lift(dt["er"]), lift(dt["ep"]), np.array([0.0, 0.0, 0.0, 1.0])
        k4 = np.concatenate([[dt["kt"]], dt["kv"]])
        frame = np.array([er4, ep4, ez4])
        # the tetrad is orthonormal under the 4 x 4 metric and the photon null
        full = np.vstack([u4[None], frame])
        dev = np.abs(full @ G @ full.T - np.diag([-1.0, 1.0, 1.0, 1.0])).max()
        # (1e-11 but for the plunge, which keeps the ISCO's E and L as the device holds them, rounded to float32: 1.3e-7 there)
        assert dev < 1e-6, (E2E[i], dev)
        assert abs(k4 @ G @ k4) < 1e-6
        fs, ks = frame @ G @ fe[i], frame @ G @ k4
        perp = fs - ((fe[i] @ G @ u4) / (k4 @ G @ u4)) * ks             # the multiple of k taken out in the gas frame
        angle = np.linalg.norm(np.cross(perp, dt["eh"])) / np.linalg.norm(perp)
        worst = max(worst, angle)
        assert angle <= 1e-6, (E2E[i], angle)
    print(f"largest angle between the transported vector and f_em in the gas frame: {worst:.2e} rad")


# ---- records of the test views ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _records(view, A, size, fov=FOV):
    cam = K.build_camera(view, fov, size[0], size[1])
    hits, mom, cnt = P.march_records(cam, A, r_inner=R_IN, r_outer=R_OUT)
    # what a device holds: float32 records
    return cam, hits.astype(np.float32), mom.astype(np.float32), cnt


def _live(cnt, K_):
    return np.arange(K_)[:, None, None] < np.minimum(cnt, K_)[None]


# ---- 3. mirror symmetry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["model", "exact"])
@pytest.mark.parametrize("A", [0.6, -0.9])
def test_mirror_symmetry(A, mode):
    """The views from (x, 0, z) and (x, 0, -z), pixel (i, j) and (i, H - 1 - j): Q equal and U negated under (b_r, b_phi, -b_z)."""
    size = (33, 9)
    cam, hits, mom, cnt = _records((6.0, 0.0, 0.5), A, size)
    cam2, hits2, mom2, cnt2 = _records((6.0, 0.0, -0.5), A, size)
    assert np.array_equal(cnt, cnt2[::-1])
    a1, b1, ok1 = P.frame_stokes(cam, hits, mom, A, mode, (0.3, 0.8, 0.5), 0.7, R_IN, R_OUT)
    a2, b2, ok2 = P.frame_stokes(cam2, hits2, mom2, A, mode, (0.3, 0.8, -0.5), 0.7, R_IN, R_OUT)
    live = _live(cnt, hits.shape[0])
    assert np.array_equal(ok1, ok2[:, ::-1]) and (ok1 & live).sum() > 100
    m = ok1 & live
    # the two marches round differently and the records are float32: 1e-5 on numbers of order one
    assert np.abs(a1 - a2[:, ::-1])[m].max() < 1e-5 and np.abs(b1 + b2[:, ::-1])[m].max() < 1e-5
    assert np.abs(b1)[m].max() > 0.1


# ---- 4. the hole that does not spin against the Schwarzschild pass ------------------------------------------------------------------
def _schwarzschild_distance(view, size, fov=FOV):
    cam, hits, mom, cnt = _records(view, 0.0, size, fov)
    live = _live(cnt, hits.shape[0])
    hx, hy = hits[..., 0].astype(np.float64), hits[..., 1].astype(np.float64)
    worst = 0.0
    w = hits[..., 2:5].astype(np.float64)          # the record's own to_cam, -dx/dl at the start of the crossing's step, as the Schwarzschild map keeps it
    for field in FIELDS:
        a, b, ok = P.frame_stokes(cam, hits, mom, 0.0, "model", field, 1.0, R_IN, R_OUT)
        sa, sb, sok = S.crossing_stokes(cam, K.pixel_rays(cam)[None], hx, hy, w, 0.0, field, 1.0, R_IN, R_OUT)
        m = ok & sok & live
        assert m.sum() >= 0.9 * live.sum()
        worst = max(worst, np.abs(a - sa)[m].max(), np.abs(b - sb)[m].max())
    return worst


def test_spin_zero_is_the_schwarzschild_model_up_to_the_camera_stretch():
    worst = {v: max(_schwarzschild_distance(v, s) for s in SIZES) for v in VIEWS}
    far = _schwarzschild_distance((100.0, 40.0, 20.0), (33, 9), fov=16.0)
    print("largest |d (Q/I, U/I)| of the A = 0 model from the Schwarzschild pass's, per view:", worst, "from (100, 40, 20):", far)
    assert max(worst.values()) <= P.SCHWARZSCHILD_DISTANCE
    assert far < 2e-2                     # what stays at a distance is the step between where a record's to_cam is taken and the hit; the stretch is gone


# ---- 5. float32 against binary64: the device's bar, and the share of single-crossing pixels ----------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_distance_and_single_crossing_share(size):
    worst = 0.0
    shares = []
    for view in VIEWS:
        for A in SPINS:
            cam, hits, mom, cnt = _records(view, A, size)
            shares.append((cnt == 1).sum() / max((cnt >= 1).sum(), 1))
            live = _live(cnt, hits.shape[0])
            for mode in ("model", "exact"):
                for field in FIELDS:
                    a64, b64, ok64 = P.frame_stokes(cam, hits, mom, A, mode, field, 1.0, R_IN, R_OUT, np.float64)
                    a32, b32, ok32 = P.frame_stokes(cam, hits, mom, A, mode, field, 1.0, R_IN, R_OUT, np.float32)
                    m = ok64 & ok32 & live
                    assert m.sum() >= 0.95 * live.sum()
                    worst = max(worst, np.abs(a64 - a32)[m].max(), np.abs(b64 - b32)[m].max())
    print(f"{size}: float32 against binary64 {worst:.3e}; single-crossing shares {min(shares):.3f} .. {max(shares):.3f}")
    assert worst <= P.F32_DISTANCE
    assert min(shares) >= (0.75 if size == (5, 3) else 0.85)
