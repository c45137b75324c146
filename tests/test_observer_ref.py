"""The moving observer's CPU reference (tests/observer_ref.py) and the host half of the feature (bhr_amd/observer.py): the
algebra of aberration and Doppler factor, the named velocities, the reference at rest against the oracle's strict frame, and
the evidence that the device test's 0.5 % cap on off pixels binds on the device alone.  No GPU."""
import numpy as np
import pytest

import observer_cases as OC
import observer_ref as R

BETAS = ((0.3, -0.4, 0.5), (0.0, 0.0, 0.9), (-0.99, 0.05, 0.0), (0.1, 0.0, 0.0), (0.5, 0.5, -0.5))


def _directions(n=500, seed=3):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


@pytest.mark.parametrize("beta", BETAS)
def test_aberrated_direction_is_unit_and_inverts(beta):
    npr = _directions()
    n, D = R.aberrate(npr, beta)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-12
    assert np.abs(R.boost_forward(n, beta) - npr).max() < 1e-12          # the forward boost of n returns n'
    assert (D > 0).all()


@pytest.mark.parametrize("speed", (0.1, 0.5, 0.9, 0.995))
def test_doppler_ahead_and_behind(speed):
    speed = float(np.float32(speed))                              # the velocity travels as three f32
    beta = np.array([0.0, speed, 0.0])
    ahead = np.sqrt((1 + speed) / (1 - speed))
    # the camera looks along n' = -(direction the photon travels): a photon that arrives from dead ahead travels against beta,
    # and the traced ray is the photon's path run backwards, so the pixel that looks ahead has n' = +beta / |beta|
    (n_a, n_b), (D_a, D_b) = R.aberrate(np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]), beta)
    assert D_a == pytest.approx(ahead, rel=1e-12) and D_b == pytest.approx(1.0 / ahead, rel=1e-12)
    assert np.allclose(n_a, [0, 1, 0], atol=1e-12) and np.allclose(n_b, [0, -1, 0], atol=1e-12)


@pytest.mark.parametrize("speed", (0.2, 0.6, 0.95))
def test_aberration_formula_about_the_velocity_axis(speed):
    """tan(theta / 2) = sqrt((1 + beta) / (1 - beta)) tan(theta' / 2), the angles from the direction of motion: the sky is
    squeezed towards it in the moving frame."""
    axis = np.array([1.0, 2.0, -0.5])
    axis /= np.linalg.norm(axis)
    npr = _directions(300, 7)
    beta = (speed * axis).astype(np.float32).astype(np.float64)   # the velocity travels as three f32
    speed, axis = np.linalg.norm(beta), beta / np.linalg.norm(beta)
    n, _ = R.aberrate(npr, beta)
    th_p, th = np.arccos(np.clip(npr @ axis, -1, 1)), np.arccos(np.clip(n @ axis, -1, 1))
    assert np.abs(np.tan(th / 2) - np.sqrt((1 + speed) / (1 - speed)) * np.tan(th_p / 2)).max() < 1e-9 * (1 + np.tan(th / 2).max())
    assert (th >= th_p - 1e-12).all()


def test_rest_is_exact_in_float32():
    npr = OC.K.pixel_rays(OC.camera(OC.VIEWS[1]), np.float32).reshape(-1, 3)
    n, D = R.aberrate(npr, (0.0, 0.0, 0.0), np.float32)
    assert n.dtype == np.float32 and np.array_equal(n, npr) and (D == np.float32(1)).all()
    c = np.random.default_rng(1).uniform(0, 1, (50, 3)).astype(np.float32)
    assert np.array_equal(R.sky_shift(c, np.ones(50, dtype=np.float32)), c)          # and the sky takes no shift at D = 1


def test_named_velocities():
    from bhr_amd import observer
    b = observer.velocity("circular", [3.0, 0.0, 0.0])
    assert np.linalg.norm(b) == pytest.approx(0.5, rel=1e-15) and np.allclose(b, [0.0, -0.5, 0.0])
    for pos in ([6.0, 0.0, 0.5], [3.0, 2.0, 0.3], [-2.0, 5.0, -1.0]):
        p = np.array(pos)
        r = np.linalg.norm(p)
        c, f = observer.velocity("circular", pos), observer.velocity("infall", pos)
        assert abs(c @ p) < 1e-15 and c[2] == 0 and np.linalg.norm(c) == pytest.approx(np.sqrt(0.5 / (r - 1)))   # tangential, horizontal
        assert np.cross(p, c)[2] < 0                              # the disk's sense: clockwise seen from +z (v_hat = r_hat x n)
        assert np.allclose(f, -np.sqrt(1 / r) * p / r, atol=1e-15)
        assert np.array_equal(observer.velocity("static", pos), np.zeros(3))
        for kind in ("circular", "infall"):                       # the reference restates them
            assert np.allclose(observer.velocity(kind, pos), R.velocity(kind, pos), atol=1e-15)
    for pos in ([1.5, 0.0, 0.0], [1.2, 0.5, 0.0], [0.0, 0.0, 4.0]):
        with pytest.raises(ValueError):
            observer.velocity("circular", pos)
    with pytest.raises(ValueError):
        observer.velocity("sideways", [6.0, 0.0, 0.5])
    for bad in ((1.0, 0.0, 0.0), (0.7, 0.7, 0.2), (float("nan"), 0.0, 0.0), (0.1, 0.2)):
        with pytest.raises(ValueError):
            observer.check_beta(bad)
    assert observer.check_beta((0.995, 0.0, 0.0)) == (0.995, 0.0, 0.0)


def test_infall_radii():
    from bhr_amd import observer
    r = observer.infall_radii(6.0, 2.0, 7)
    assert r[0] == 6.0 and r[-1] == 2.0 and (np.diff(r) < 0).all()
    assert np.allclose(np.diff(r ** 1.5), (2.0 ** 1.5 - 6.0 ** 1.5) / 6)          # uniform in proper time: d tau = -sqrt(r) dr
    assert list(observer.infall_radii(5.0, 2.0, 1)) == [5.0]
    with pytest.raises(ValueError):
        observer.infall_radii(5.0, 2.0, 0)


# ---- the reference at rest against the oracle's strict frame -------------------------------------------------------------------
# Measured (per-channel RMSE of the float32 reference against OracleRenderer's layers, 96 x 64, the four cases below): BG at most
# 4.6e-7, DISK at most 1.05e-6, the step totals equal.  The two differ in libm (the oracle's C against NumPy's float32 loops);
# a tie of reference to reference gets four times the measured distance, as elsewhere in this project (DESIGN.md "Observer").
ORACLE_BAR = {"bg": 4 * 4.6e-7, "disk": 4 * 1.05e-6}


@pytest.mark.parametrize("case", OC.AT_REST, ids=lambda c: c.name)
def test_reference_at_rest_is_the_oracles_strict_frame(case, oracle):
    sky, tex = OC.scene()
    o = oracle.OracleRenderer(OC.W, OC.H, sky, tex, step_size=OC.STEP, r_max=OC.R_MAX, r_disk_inner=OC.R_INNER,
                              r_disk_outer=OC.R_OUTER, disk_tilt=case.tilt)
    _, bg, disk, _ = o.render(list(case.view), OC.FOV, skip_bloom=True, parts=True)
    r32 = OC.reference(case, np.float32)
    d_bg, d_disk = OC.rmse(r32["bg"], bg.transpose(1, 0, 2)), OC.rmse(r32["disk"], disk.transpose(1, 0, 2))
    print(f"{case.name}: float32 reference against the oracle: BG {d_bg}, DISK {d_disk}, steps {int(r32['steps'].sum())} / {o.last_total_steps}")
    assert (d_bg <= ORACLE_BAR["bg"]).all() and (d_disk <= ORACLE_BAR["disk"]).all()
    assert int(r32["steps"].sum()) == o.last_total_steps


@pytest.mark.parametrize("case", OC.CASES, ids=lambda c: c.name)
def test_float32_reference_stays_under_the_off_pixel_cap(case):
    """The device test allows 0.5 % of the pixels to be off by more than 1e-3; the float32 reference itself stays under it on
    every case, so the cap binds on the device alone."""
    r32, r64 = OC.reference(case, np.float32), OC.reference(case, np.float64)
    share = OC.off_share((r32["bg"], r32["disk"]), (r64["bg"], r64["disk"]))
    print(f"{case.name}: {share:.5f} of the pixels differ by more than 1e-3 between the float32 and binary64 references")
    assert share < 0.005
    assert np.isfinite(r64["bg"]).all() and np.isfinite(r64["disk"]).all()
    assert r64["D"].max() > 1.0                                   # every case has pixels that look ahead of the motion
