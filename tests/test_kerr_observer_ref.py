"""The Kerr camera's CPU reference (tests/kerr_observer_ref.py) and the product's named velocities (bhr_amd.observer.kerr_velocity):
the velocities against a table computed from the 4 x 4 metric and against that metric itself, the reference at rest against the
references of the Kerr march, at A = 0 against the Schwarzschild observer's and projection's references (printed: twice that
distance is a bar of tests/test_gpu_kerr_observer.py), and what binary32 costs on every shared case."""
import math

import numpy as np
import pytest

import kerr_cases as KC
import kerr_observer_cases as VC
import kerr_observer_ref as V
import kerr_redshift_ref as X
import kerr_ref as K

# beta of an equatorial camera at Kerr-Schild radius r (position (sqrt(r^2 + a^2), 0, 0)), computed from the 4 x 4 metric
TABLE = (("circular", 0.6, 3.0, 0.474668642702248), ("circular", -0.9, 2.0, 0.9574723922358599), ("circular", 0.998, 6.0, 0.30864539905969174),
         ("zamo", 0.998, 2.0, 0.1663702716342419), ("zamo", -0.9, 3.0, -0.06022930788591241))


def _equatorial(r, A):
    return (math.sqrt(r * r + (0.5 * A) ** 2), 0.0, 0.0)


@pytest.mark.parametrize("kind,A,r,beta", TABLE)
def test_named_velocities_against_the_table(kind, A, r, beta):
    from bhr_amd.observer import kerr_velocity
    pos = _equatorial(r, A)
    b = kerr_velocity(kind, pos, A)
    assert b[0] == 0 and b[2] == 0
    assert abs(-b[1] - beta) <= 1e-12                      # v_hat = (y, -x, 0) / rho = (0, -1, 0) here
    assert np.abs(V.velocity(kind, pos, A) - b).max() <= 1e-12


@pytest.mark.parametrize("kind", ("circular", "zamo"))
@pytest.mark.parametrize("A", (0.6, -0.9, 0.998, 0.0))
@pytest.mark.parametrize("pos", ((3.0, 2.0, 0.0), (-2.5, 4.0, 0.0), (3.0, 2.0, 0.3), (0.4, -0.3, 5.0)))
def test_gamma_is_minus_u_dot_u_static_in_the_4x4_metric(kind, A, pos):
    """gamma = -u.u_static with both four-velocities normalised in the Kerr-Schild metric written out as a 4 x 4 matrix
    (kerr_observer_ref.ks_metric), against the product's closed form in Boyer-Lindquist components."""
    from bhr_amd.observer import kerr_velocity
    if kind == "circular" and pos[2] != 0:
        with pytest.raises(ValueError, match="equatorial"):
            kerr_velocity(kind, pos, A)
        return
    b = kerr_velocity(kind, pos, A)
    om = V.omega_of(kind, pos, A)
    gam = V.orbit_gamma(pos, A, om)
    assert abs(1.0 / math.sqrt(1.0 - float(b @ b)) - gam) <= 1e-12 * gam
    assert abs(float(b @ b) - (1.0 - 1.0 / gam ** 2)) <= 1e-12       # (beta itself from gamma loses half the digits at beta -> 0)
    rho = math.hypot(pos[0], pos[1])
    v_hat = np.array([pos[1] / rho, -pos[0] / rho, 0.0])
    assert np.abs(b - math.copysign(math.sqrt(float(b @ b)), om) * v_hat).max() <= 1e-15        # along v_hat, in omega's sense
    if kind == "zamo":
        assert math.copysign(1.0, float(b @ v_hat)) == math.copysign(1.0, A) or A == 0      # dragged in the hole's sense
        assert A != 0 or np.all(b == 0)


def test_spin_zero_is_the_schwarzschild_observers_velocity():
    from bhr_amd.observer import kerr_velocity, velocity
    for pos in ((3.0, 2.0, 0.0), (0.0, -6.0, 0.0), (1.2, 1.2, 0.0)):
        assert np.abs(kerr_velocity("circular", pos, 0.0) - velocity("circular", pos)).max() <= 1e-15
        assert np.all(kerr_velocity("static", pos, 0.0) == 0) and np.all(kerr_velocity("zamo", pos, 0.0) == 0)
    assert np.all(kerr_velocity("zamo", (0.0, 0.0, 3.0), 0.9) == 0)          # on the axis


def test_velocities_that_are_refused():
    from bhr_amd.observer import kerr_velocity
    for args, word in ((("infall", (6, 0, 0), 0.5), "infall"), (("circular", (3, 2, 0.3), 0.5), "equatorial"), (("orbit", (6, 0, 0), 0.5), "one of"),
                       (("circular", (1.3, 0, 0), -0.9), "no such orbit|at most"), (("circular", (2.01, 0, 0), -0.9), "at most"),
                       (("zamo", (1.01, 0, 0), 0.998), "static limit"), (("zamo", (6, 0, 0), 1.2), "spin")):
        with pytest.raises(ValueError, match=word):
            kerr_velocity(*args)


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("redshift", ("model", "exact"))
def test_at_rest_under_the_pinhole_it_is_the_kerr_reference(redshift, dtype):
    sky, tex = KC.scene()
    A, view = 0.9, KC.VIEWS[1]
    cam = K.build_camera(list(view), KC.FOV, 48, 32, KC.R_MAX)
    kw = dict(h_base=KC.STEP, r_inner=KC.R_INNER, r_outer=KC.R_OUTER, dtype=dtype)
    want = (X.render if redshift == "exact" else K.render)(cam, A, sky, tex, **kw)
    for beta, shift in ((None, True), ((0.0, 0.0, 0.0), True), ((0.0, 0.0, 0.0), False)):
        got = V.render(cam, A, sky, tex, beta=beta, sky_shift_on=shift, redshift=redshift, **kw)
        for k in ("bg", "disk", "final", "fate", "n_hits", "steps"):
            assert np.array_equal(got[k], want[k]), (k, beta, shift)
        assert np.all(got["D"] == 1) and got["inside"].all()
    assert want["disk"].max() > 0 and want["bg"].max() > 0


@pytest.mark.parametrize("case", VC.SCHWARZSCHILD, ids=lambda c: c.id)
def test_at_spin_zero_its_distance_from_the_schwarzschild_references(case):
    """Printed: twice these distances (floor 1e-4) bar the forced Kerr camera against bhr_render_observer / bhr_render_projected."""
    d, share = VC.schwarzschild_distance(case)
    print(f"{case.id}: kerr_observer_ref (A = 0, binary64) against the Schwarzschild reference: {d}; fate / crossing count differs on {share:.3%}")
    assert share <= 0.005
    assert all(v <= 5e-3 for v in d.values())             # two integrators of one geodesic at h = 0.1: the same picture


@pytest.mark.parametrize("case", VC.REFERENCE + VC.SCHWARZSCHILD, ids=lambda c: c.id)
def test_float32_keeps_fates_and_crossings(case):
    r64, r32 = VC.reference(case, np.float64), VC.reference(case, np.float32)
    d, share = VC.float32_distance(case)
    steps = abs(int(r32["steps"].sum()) - int(r64["steps"].sum())) / int(r64["steps"].sum())
    print(f"{case.id}: float32 against binary64: {d}; fate / crossing count differs on {share:.3%}; step totals differ by {steps:.3g}")
    assert share <= 0.005
    assert r64["disk"].max() > 0 and r64["bg"].max() > 0
    if case.projection == "fisheye":
        assert not r64["inside"].all() and np.all(r64["bg"][~r64["inside"]] == 0) and np.all(r64["steps"][~r64["inside"]] == 0)
    if case.beta is not None:
        assert np.ptp(r64["D"][r64["inside"]]) > 0.05      # the camera really moves
