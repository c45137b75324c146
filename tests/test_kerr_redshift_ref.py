"""The CPU reference of the exact Kerr disk redshift (tests/kerr_redshift_ref.py) against what can be known without it: the
march of kerr_ref, the literal contraction with the 4 x 4 Kerr-Schild metric and its numerical inverse, continuity at the
ISCO, the view from the axis, the order of the interpolated hit state, and the sense of the brightness asymmetry.  No GPU."""
import functools

import numpy as np
import pytest

import kerr_cases as KC
import kerr_redshift_ref as R
import kerr_ref as K

SPINS = [0.0, 0.6, -0.9, 0.998]
VIEW = (6.0, 0.0, 0.5)


# ----------------------------------------------------------------------------------------------- (a) the march
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("view", KC.VIEWS, ids=lambda v: f"pov{v[0]:g}_{v[1]:g}")
def test_march_is_kerr_refs(view, dtype):
    """Fates, steps, crossing counts and hit points equal kerr_ref.march's exactly (a 24 x 16 grid of the device test's views)."""
    cam = K.build_camera(list(view), KC.FOV, 24, 16, KC.R_MAX)
    d = K.pixel_rays(cam, dtype).reshape(-1, 3)
    x0 = cam["pos"].astype(dtype)
    for A in SPINS:
        kw = dict(h_base=KC.STEP, r_escape=cam["r_escape"], r_inner=KC.R_INNER, r_outer=KC.R_OUTER, dtype=dtype)
        want, got = K.march(x0, d, A, **kw), R.march(x0, d, A, **kw)
        for k in ("fate", "steps", "n_hits", "esc_dir"):
            assert np.array_equal(want[k], got[k]), (A, k)
        assert want["hits"].shape == got["hits"].shape and want["hits"].shape[0] > 20
        assert np.array_equal(want["hits"][:, :4], got["hits"][:, :4]), A


# ----------------------------------------------------------------------------------------------- (b) the closed forms
def _metric(x, a):
    """g_{mu nu} = eta + f l l with l_mu = (1, l), per point (n, 4, 4); literal."""
    _, f, l = K.geometry(x, a)
    lc = np.concatenate([np.ones((x.shape[0], 1)), l], axis=1)
    eta = np.diag([-1.0, 1.0, 1.0, 1.0])
    return eta[None] + f[:, None, None] * lc[:, :, None] * lc[:, None, :]


def _equatorial_photons(A, n, seed, r_lo, r_hi):
    """n equatorial points with r in [r_lo, r_hi] and a null covariant momentum (-1, p) at each."""
    rng = np.random.default_rng(seed)
    a = A * K.M
    r = rng.uniform(r_lo, r_hi, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    rho = np.sqrt(r * r + a * a)
    x = np.stack([rho * np.cos(phi), rho * np.sin(phi), np.zeros(n)], axis=1)
    # p = s d with p.p - 1 - f (1 + l.p)^2 = 0: a quadratic in s with two real roots wherever the point lies (the camera's
    # K.initial_momentum has none inside the ergosphere)
    d = rng.normal(size=(4 * n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d = d[:n]
    _, f, l = K.geometry(x, a)
    c = (l * d).sum(1)
    s = (1.0 + f) / (np.sqrt(1.0 + f * (1.0 - c * c)) - f * c)          # the root that is > 0 for f c^2 < 1, in its stable form
    p = s[:, None] * d
    assert (np.abs(K.hamiltonian(x, p, a)) < 1e-13 * (1.0 + (p * p).sum(1))).all() and np.abs(K.ks_radius(x, a) - r).max() < 1e-12
    return x, p, r


def _photon_numbers(x, p, r, a):
    rho = np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2)
    lz = x[:, 0] * p[:, 1] - x[:, 1] * p[:, 0]
    P = (x[:, 0] * p[:, 0] + x[:, 1] * p[:, 1]) / rho
    U = 1.0 + (r * P - a * lz / rho) / rho
    return rho, lz, P, U


@pytest.mark.parametrize("A", SPINS)
def test_closed_forms_equal_the_metric_contraction(A):
    a = A * K.M
    r_isco, E_i, L_i = R.isco_orbit(A)
    r_ph = K.r_photon(A, A >= 0)
    pc = np.concatenate  # noqa: E731
    # -- the circular branch, outside the photon orbit of the disk's sense
    x, p, r = _equatorial_photons(A, 50, 11, 1.05 * r_ph, 15.0)
    rho, lz, P, U = _photon_numbers(x, p, r, a)
    _, _, l = K.geometry(x, a)
    assert np.abs(U - (1.0 + (l * p).sum(1))).max() < 1e-12                 # U is 1 + l.p in the plane
    g = _metric(x, a)
    om = R.omega_exact(r, a)
    vel = np.stack([np.ones_like(r), -om * x[:, 1], om * x[:, 0], np.zeros_like(r)], axis=1)     # (1, Omega e_phi rho)
    norm = np.einsum("ni,nij,nj->n", vel, g, vel)
    ut = 1.0 / np.sqrt(-norm)
    u_up = ut[:, None] * vel
    p_cov = pc([-np.ones((50, 1)), p], axis=1)
    nu_lit = -(p_cov * u_up).sum(1)
    err_ut = np.abs(ut - 1.0 / np.sqrt(R.circular_radicand(r, a, om))).max()
    err_nu = np.abs(nu_lit - R.nu_em_circular(r, a, lz, om)).max()
    u_dn = np.einsum("nij,nj->ni", g, u_up)
    E_b, L_b = R.bardeen_energy_momentum(r, a)
    err_E = np.abs(-u_dn[:, 0] - E_b).max()
    err_L = np.abs((x[:, 0] * u_dn[:, 2] - x[:, 1] * u_dn[:, 1]) - L_b).max()
    # -- the plunging branch, between the horizon and the ISCO
    x, p, r = _equatorial_photons(A, 50, 12, 1.02 * K.r_plus(A), r_isco)
    rho, lz, P, U = _photon_numbers(x, p, r, a)
    ginv = np.linalg.inv(_metric(x, a))
    w, S = R.plunge_velocity(r, a, r_isco, E_i, L_i)
    # the discriminant's factorised form (what plunge_velocity evaluates) is the literal qb^2 - 4 qa qc
    err_disc = np.abs(R.plunge_discriminant(r, a, r_isco, E_i, L_i) - (2.0 * (w - S / rho)) ** 2).max()
    e_rho = np.stack([x[:, 0], x[:, 1]], axis=1) / rho[:, None]
    e_phi = np.stack([-x[:, 1], x[:, 0]], axis=1) / rho[:, None]
    sp = (L_i / rho)[:, None] * e_phi + w[:, None] * e_rho
    u_dn = pc([np.full((50, 1), -E_i), sp, np.zeros((50, 1))], axis=1)
    u_up = np.einsum("nij,nj->ni", ginv, u_dn)
    p_cov = pc([-np.ones((50, 1)), p], axis=1)
    err_norm = np.abs(np.einsum("ni,ni->n", u_dn, u_up) + 1.0).max()
    radial = (u_up[:, 1:3] * e_rho).sum(1)
    err_rad = np.abs(radial - (w - S / rho)).max()
    err_nu_p = np.abs(-(p_cov * u_up).sum(1) - R.nu_em_plunge(r, a, lz, P, U, r_isco, E_i, L_i)).max()
    print(f"A={A}: u^t {err_ut:.2g}, nu_em circular {err_nu:.2g}, E {err_E:.2g}, L {err_L:.2g}; plunge: norm {err_norm:.2g}, "
          f"radial {err_rad:.2g}, nu_em {err_nu_p:.2g}, discriminant {err_disc:.2g}, largest u^rho {radial.max():.3g}")
    assert max(err_ut, err_nu, err_E, err_L, err_nu_p, err_norm, err_rad, err_disc) < 1e-12
    assert (radial <= 1e-7).all() and (u_up[:, 0] > 0).all()                 # inward and future-directed


# ----------------------------------------------------------------------------------------------- (c) continuity at the ISCO
@pytest.mark.parametrize("A", SPINS)
def test_g_is_continuous_across_the_isco(A):
    a = A * K.M
    r_isco, E, L = R.isco_orbit(A)
    x, p, r = _equatorial_photons(A, 50, 13, r_isco, r_isco)
    rho, lz, P, U = _photon_numbers(x, p, r, a)
    nu_c = R.nu_em_circular(r, a, lz, R.omega_exact(r, a))
    nu_p = R.nu_em_plunge(r, a, lz, P, U, r_isco, E, L)
    nu_obs = R.nu_observer(np.array(VIEW), a, np.float64)
    gap = np.abs(nu_obs / nu_c - nu_obs / nu_p).max()
    guard = np.abs(nu_obs / nu_c - nu_obs / R.nu_em_circular(r, a, lz, K.omega_kerr(r, a))).max()
    print(f"A={A}: r_isco {r_isco:.6f}, E {E:.9f}, L {L:.9f}: |g_circular - g_plunge| at r_isco {gap:.3g} "
          f"(the 1e-6 guard of omega_kerr moves g_circular by {guard:.3g})")
    assert gap < 1e-9


# ----------------------------------------------------------------------------------------------- (d) the axis
@pytest.mark.parametrize("A", SPINS)
def test_from_the_axis_g_is_the_emitters_time_dilation(A):
    a = A * K.M
    cam = K.build_camera([0.0, 0.0, 8.0], 120.0, 12, 12, KC.R_MAX)
    d = K.pixel_rays(cam).reshape(-1, 3)
    x0 = cam["pos"].astype(np.float64)
    m = R.march(x0, d, A, h_base=0.05, r_escape=cam["r_escape"], r_inner=0.5, r_outer=KC.R_OUTER)
    rows = m["hits"]
    assert rows.shape[0] > 30
    hx, hy, lz, P, U = (rows[:, c] for c in range(2, 7))
    # L_z = 0 at the camera and conserved; the march keeps it to its own error (measured at this step: 2.1e-5 at most)
    assert np.abs(lz).max() < 1e-4
    isco = R.isco_orbit(A)
    r = np.sqrt(hx * hx + hy * hy - a * a)
    out = r >= isco[0]
    assert out.sum() > 10
    om = K.omega_kerr(r[out], a)
    f_cam = K.geometry(x0[None], a)[1][0]
    want = np.sqrt(R.circular_radicand(r[out], a, om)) / np.sqrt(1.0 - f_cam)
    assert (want < K.G_FACTOR_CAP).all()
    zero = np.zeros_like(lz)
    g0 = R.g_exact(hx, hy, zero, P, U, a, cam["pos"], isco)[out]
    g = R.g_exact(hx, hy, lz, P, U, a, cam["pos"], isco)[out]
    assert np.abs(g0 - want).max() < 1e-12
    assert np.abs(g - want / (1.0 - om * lz[out])).max() < 1e-12           # ... and with the L_z the march arrived with
    assert np.abs(g - want).max() < 2.0 * np.abs(om * lz[out]).max()


# ----------------------------------------------------------------------------------------------- (e) order of the hit state
@functools.lru_cache(maxsize=None)
def _first_g(A, step):
    sky, tex = np.ones((4, 8, 3), dtype=np.float32), np.ones((4, 8, 4), dtype=np.float32)
    cam = K.build_camera(list(VIEW), KC.FOV, 8, 8, KC.R_MAX)
    out = R.render(cam, A, sky, tex, h_base=step, r_inner=KC.R_INNER, r_outer=KC.R_OUTER)
    return out["first_g"]


@pytest.mark.parametrize("A", [0.6, -0.9])
def test_hit_state_is_second_order_in_the_step(A):
    fine = _first_g(A, 0.0125)
    e1, e2 = np.abs(_first_g(A, 0.1) - fine), np.abs(_first_g(A, 0.05) - fine)
    both = np.isfinite(e1) & np.isfinite(e2) & (fine < K.G_FACTOR_CAP)
    m1, m2 = np.median(e1[both]), np.median(e2[both])
    print(f"A={A}: {int(both.sum())} first crossings, median |g - g(0.0125)|: step 0.1 {m1:.3g}, step 0.05 {m2:.3g}, ratio {m1 / m2:.2f}")
    assert both.sum() >= 10
    assert m1 >= 3.0 * m2


# ----------------------------------------------------------------------------------------------- (f) sense
def test_brighter_side_is_the_models():
    case = (0.6, VIEW)
    A, view = case
    sky, tex = KC.scene()
    cam = K.build_camera(list(view), KC.FOV, 48, 32, KC.R_MAX)
    kw = dict(h_base=KC.STEP, r_inner=KC.R_INNER, r_outer=KC.R_OUTER)
    model = K.render(cam, A, sky, tex, **kw)["disk"]
    exact = R.render(cam, A, sky, tex, **kw)["disk"]
    half = lambda im: (float(im[:, :24].sum()), float(im[:, 24:].sum()))    # noqa: E731
    (ml, mr), (el, er) = half(model), half(exact)
    print(f"DISK layer left / right: model {ml:.2f} / {mr:.2f}, exact {el:.2f} / {er:.2f}")
    assert abs(ml - mr) > 0.05 * (ml + mr) and abs(el - er) > 0.05 * (el + er)
    assert (ml > mr) == (el > er)
    assert not np.array_equal(model, exact)
