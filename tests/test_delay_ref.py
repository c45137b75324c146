"""The light delay's CPU reference (tests/delay_ref.py) held to what is known without it: the closed form of a radial ray, an
independent integration of the four-dimensional null geodesic, the undelayed reference at scale 0, and the evidence that the
device test's 0.5 % cap on off pixels binds on the device alone.  No GPU."""
import numpy as np
import pytest

import delay_cases as DC
import delay_ref as D
import kerr_ref as K
import observer_ref as R


# ---- the radial ray -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_cam", (3.0, 6.0))
def test_radial_ray_has_the_closed_form(r_cam):
    """L = 0, E = 1, dt/dr = r / (r - 1): T(r) = (r - r_cam) + ln((r - 1) / (r_cam - 1)).  The ray leaves the plane z = 0 at
    once (no crossing) and ends beyond r_escape; the time at its last step is held at the radius of that step."""
    x0 = np.array([0.48, 0.6, 0.64]) * r_cam                      # a unit vector off every axis and off the plane
    m = D.march(x0, (x0 / np.linalg.norm(x0))[None, :], h_base=0.1, r_escape=2.0 * r_cam)
    r = float(m["r_end"][0])
    want = (r - r_cam) + np.log((r - 1.0) / (r_cam - 1.0))
    assert m["fate"][0] == 1 and r > 2.0 * r_cam and m["hits"].shape[0] == 0
    assert float(m["E"][0]) == pytest.approx(1.0, abs=1e-15)
    print(f"[delay] radial ray from {r_cam}: T = {float(m['T'][0]):.12f} at r = {r:.6f}, closed form {want:.12f}")
    assert float(m["T"][0]) == pytest.approx(want, rel=1e-6)


# ---- the independent integration --------------------------------------------------------------------------------------------------
# eight rays of the first two views whose first crossing lies well inside the disk: near side, far side (behind the hole, bent
# over it), both tilts
GEODESIC_RAYS = ((DC.VIEWS[0], 0.0, (40, 48)), (DC.VIEWS[0], 0.0, (9, 37)), (DC.VIEWS[0], 0.0, (39, 15)), (DC.VIEWS[0], 0.0, (63, 30)),
                 (DC.VIEWS[0], 25.0, (47, 39)), (DC.VIEWS[0], 25.0, (33, 37)), (DC.VIEWS[1], 0.0, (81, 10)), (DC.VIEWS[1], 25.0, (89, 29)))


@pytest.mark.parametrize("view,tilt,pixel", GEODESIC_RAYS, ids=lambda v: str(v).replace(" ", ""))
def test_first_crossing_time_agrees_with_the_geodesic(view, tilt, pixel):
    """The reference's T at a ray's first crossing against t of the four-dimensional geodesic (delay_ref.geodesic_first_crossing,
    which shares only the step rule with the march), integrated at a step ten times finer than the march's.

    The bar, from three terms that do not come from the reference's result:
      * the fine integration's own error, by Richardson from halving its step once: e_fine = 16/15 |t(h/10) - t(h/20)|;
      * the reference's integration at the ten times coarser step h: RK4 and Simpson's rule are fourth order like the fine
        integration, so 1e4 e_fine, twice that because the path and the quadrature each contribute a term of the order;
      * the crossing inside its step: the march places it by linear interpolation of the plane function and takes T linear in
        the step.  A linear interpolant over a step h is off by at most h^2 / 8 max|T''|, and T'' = E w'(r) dr/dl with E <= 1,
        |dr/dl| <= 1, |w'| = 1 / (r - 1)^2 -- at the smallest radius of the step, r_hit - h; the root of the plane function moves
        by a third-order term (the acceleration is radial, so its component across the plane vanishes on the plane), which
        h^3 / 8 * 1.5 L^2 / r^5 * w(r) bounds with L^2 <= r_cam^2.
    h is the march's step at the crossing, 0.1 dt_fac(r_hit + 0.5) (dt_fac grows with r there and a step is shorter than 0.5)."""
    i, j = pixel
    cam = DC.camera(view)
    d = K.pixel_rays(cam)[j, i]
    x0 = cam["pos"].astype(np.float64)
    m = D.march(x0, d[None, :], h_base=DC.STEP, r_escape=cam["r_escape"], r_inner=DC.R_INNER, r_outer=DC.R_OUTER, tilt_deg=tilt)
    assert m["n_hits"][0] >= 1, "the test's ray must cross the disk"
    row = m["hits"][0]
    assert row[1] == 0
    tan_t = np.tan(np.radians(tilt))
    t_ref, hit = float(row[7]), np.array([row[2], row[3], row[3] * tan_t])
    fine = D.geodesic_first_crossing(x0, d, DC.STEP / 10, tilt, DC.R_INNER, DC.R_OUTER)
    finer = D.geodesic_first_crossing(x0, d, DC.STEP / 20, tilt, DC.R_INNER, DC.R_OUTER)
    assert fine is not None and finer is not None
    e_fine = 16.0 / 15.0 * abs(fine[0] - finer[0])
    r_hit = float(np.linalg.norm(hit))
    h = DC.STEP * float(K.dt_fac(np.array([r_hit + 0.5]))[0])
    r_min = r_hit - h
    assert r_min > 1.5, "the test's ray must cross away from the horizon"
    r_cam2 = float(x0 @ x0)
    interp = h * h / 8.0 / (r_min - 1.0) ** 2 + h ** 3 / 8.0 * 1.5 * r_cam2 / r_min ** 5 * (r_min / (r_min - 1.0))
    bar = 2.0e4 * e_fine + interp + 1e-9
    print(f"[delay] view {view} tilt {tilt} pixel {pixel}: T_hit {t_ref:.9f}, geodesic {fine[0]:.9f} (halved step {finer[0]:.9f}), "
          f"off by {abs(t_ref - fine[0]):.3e}, bar {bar:.3e} (interpolation {interp:.3e}, integration {2e4 * e_fine:.3e}); hit at r = {r_hit:.4f}, "
          f"the geodesic's {np.linalg.norm(fine[1]):.4f}")
    assert np.linalg.norm(fine[1] - hit) < 5e-3                  # the same crossing
    assert abs(t_ref - fine[0]) <= bar


# ---- scale 0 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("binary64", "float32"))
def test_scale_zero_is_the_undelayed_reference(dtype):
    """The stepping is observer_ref's at beta = 0: with scale 0 the frame, the step counts and the crossings are its, exactly."""
    case = DC.CASES[-1]._replace(tilt=25.0)                       # the noisy texture, t_offset 7.3, a tilted disk
    sky, tex = DC.scene(case.texture)
    cam = DC.camera(case.view)
    t_off = np.float32(case.t_offset)
    got = D.render(cam, 0.0, sky, tex, h_base=DC.STEP, r_inner=DC.R_INNER, r_outer=DC.R_OUTER, tilt_deg=case.tilt, t_offset=t_off, dtype=dtype)
    want = R.render(cam, (0.0, 0.0, 0.0), sky, tex, h_base=DC.STEP, r_inner=DC.R_INNER, r_outer=DC.R_OUTER, tilt_deg=case.tilt,
                    t_offset=t_off, sky_shift_on=False, dtype=dtype)
    for k in ("bg", "disk", "fate", "n_hits", "steps"):
        assert np.array_equal(got[k], want[k]), k
    assert got["disk"].max() > 0 and (got["n_hits"] >= 2).any()
    # The delay rolls the texture and nothing else.  BG is the sky through 1 - alpha of the crossings: it is the same bits where a
    # ray crosses no disk, stays within the sampler's rounding (DC.BG_ROUNDING) where the texture's alpha does not depend on phi
    # (the smooth texture), and moves with the disk where it does (the noisy one).
    smooth = DC.CASES[1]
    delayed, undelayed = DC.reference(smooth, dtype), DC.reference(smooth, dtype, scale=0.0)
    clear = undelayed["n_hits"] == 0
    assert np.array_equal(delayed["steps"], undelayed["steps"]) and np.array_equal(delayed["n_hits"], undelayed["n_hits"])
    assert np.array_equal(delayed["bg"][clear], undelayed["bg"][clear]) and clear.any() and not clear.all()
    assert np.abs(delayed["bg"].astype(np.float64) - undelayed["bg"]).max() <= DC.BG_ROUNDING
    assert not np.array_equal(delayed["disk"], undelayed["disk"])
    noisy = DC.reference(case, dtype)
    assert np.array_equal(noisy["steps"], want["steps"]) and not np.array_equal(noisy["disk"], want["disk"])
    moved = (noisy["bg"] != want["bg"]).any(axis=2)
    assert moved.any() and (want["n_hits"][moved] > 0).all()


# ---- every case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.name)
def test_times_are_finite_and_float32_stays_under_the_cap(case):
    """T is finite wherever a crossing is parked -- the rays that end in the hole included -- and positive and ordered along a
    ray; and the float32 reference keeps at most 0.5 % of the pixels off by more than 1e-3 from its binary64 run, so the device
    test's cap binds on the device alone."""
    r64, r32 = DC.reference(case, np.float64), DC.reference(case, np.float32)
    for ref in (r64, r32):
        rows = ref["hits"]
        assert rows.shape[0] > 0 and np.isfinite(rows[:, 7]).all() and (rows[:, 7] > 0).all()
        assert np.isfinite(ref["T"]).all()
        captured = ref["fate"].reshape(-1)[rows[:, 0].astype(np.int64)] == 0
        assert captured.any(), "no captured ray crosses the disk in this case"
        second = rows[rows[:, 1] == 1]
        first = {int(r[0]): r[7] for r in rows[rows[:, 1] == 0]}
        assert all(r[7] > first[int(r[0])] for r in second)
    share = DC.off_share((r32["bg"], r32["disk"]), (r64["bg"], r64["disk"]))
    print(f"[delay] {case.name}: float32 reference off binary64 in {share:.5f} of the pixels; RMSE bg {DC.rmse(r32['bg'], r64['bg'])}, "
          f"disk {DC.rmse(r32['disk'], r64['disk'])}; T reaches {float(r64['hits'][:, 7].max()):.2f}; {int((r64['n_hits'] >= 2).sum())} pixels with a second image")
    assert share <= 0.005
    assert int(r32["steps"].sum()) == pytest.approx(int(r64["steps"].sum()), rel=2e-4)
