"""The inputs of tests/test_gpu_observer_edges.py and tests/test_gpu_projection_edges.py are fair: on every case the float32 run
of the reference stays within the device's caps against its binary64 run, so those caps bind on the device alone; every frame
holds what its case claims; and each case exercises what it is there for -- the radial cases have a ray with L = 0, the clamp
cases leave [0.1, 1.5] on rays that reach the sky, the roll moves the disk and no ray, the many-crossing cases have rays with
three and more crossings whose late crossings show.  No device.

Where a premise failed, the input moved and not the cap.  One did: from (6, 0, 0.5) the middle pixel of an odd frame is radial
to 2e-6 in float32 and not exactly, so the two radial cases (33 x 33 pinhole, 0.9 ahead; fisheye 180, 33 x 33, at rest) look
from (6, 0, 0.75), where d x p is exactly 0 (tests/observer_edge_cases.py: RADIAL_VIEW).  Every other case is as planned."""
import numpy as np
import pytest

import observer_edge_cases as EC
import observer_ref as R
import projection_ref as P

ids = lambda c: c.name


@pytest.mark.parametrize("case", EC.ALL, ids=ids)
def test_float32_reference_is_within_the_device_caps(case):
    r64, r32 = EC.reference(case, np.float64), EC.reference(case, np.float32)
    off = EC.off_pixels((r32["bg"], r32["disk"]), (r64["bg"], r64["disk"]))
    s32, s64 = int(r32["steps"].sum()), int(r64["steps"].sum())
    print(f"[edges_ref] {case.name}: {off} of {case.pixels} pixels off by more than 1e-3 (at most {EC.off_cap(case.pixels):g}); RMSE bg "
          f"{EC.rmse(r32['bg'], r64['bg']).max():.1e} disk {EC.rmse(r32['disk'], r64['disk']).max():.1e}; steps float32 {s32} binary64 {s64}")
    assert off <= EC.off_cap(case.pixels)
    assert abs(s32 - s64) <= EC.steps_bar(s64)
    assert np.array_equal(r32["inside"], r64["inside"])
    assert r64["inside"].all() == (case.kind != P.FISHEYE or case.size == (1, 1))      # a fisheye frame has corners outside its circle
    assert np.array_equal(r32["fate"] == 2, r64["fate"] == 2)          # no live ray runs out of iterations in one run alone
    off_circle = ~r64["inside"]
    for r in (r64, r32):
        assert all(np.isfinite(r[k]).all() for k in ("bg", "disk", "D", "n"))
        assert (r["bg"][off_circle] == 0).all() and (r["disk"][off_circle] == 0).all() and (r["steps"][off_circle] == 0).all()
        assert (r["steps"][r["inside"]] > 0).all()


@pytest.mark.parametrize("case", EC.ALL, ids=ids)
def test_frames_hold_what_their_cases_claim(case):
    r64 = EC.reference(case)
    live = r64["inside"]
    captured, escaped = int((r64["fate"][live] == 0).sum()), int((r64["fate"][live] == 1).sum())
    print(f"[edges_ref] {case.name}: {captured} captured, {escaped} escaped, DISK up to {r64['disk'].max():.3f}, BG up to {r64['bg'].max():.3f}, "
          f"D {r64['D'].min():.3f} .. {r64['D'].max():.3f}, at most {int(r64['n_hits'].max())} crossings")
    assert r64["disk"].max() > 0 and r64["bg"].max() > 0
    assert captured + escaped == int(live.sum())                       # no ray runs out of iterations
    assert case.fates in ("both", "escaped")
    assert escaped > 0 and (captured > 0) == (case.fates == "both")
    if case.beta is not None and any(case.beta):
        assert r64["D"].min() < 1.0 or r64["D"].max() > 1.0           # the camera moves
    assert (r64["bg"].shape, r64["disk"].shape) == ((case.size[1], case.size[0], 3),) * 2


def test_the_case_tables_are_the_planned_ones():
    """Sizes that are no multiple of the 8 x 8 tile, one pixel, one column, one tile row, more than one tile each way."""
    sizes = {c.size for c in EC.RAGGED + EC.PROJECTIONS}
    assert {(61, 43), (33, 33), (5, 3), (1, 1), (1, 7), (130, 3), (9, 65), (61, 31), (7, 3), (130, 5), (45, 29), (29, 45), (31, 31)} <= sizes
    assert all(c.beta is not None and any(c.beta) for c in EC.RAGGED)              # each ragged pinhole frame moves
    assert len({c.name for c in EC.ALL}) == len(EC.ALL) == 8 + 3 + 7 + 13 + 2 + 2
    for c in EC.CLAMPS + EC.CLAMPS_PROJECTED:
        assert 0.9949 < np.linalg.norm(np.float32(c.beta).astype(np.float64)) <= R.BETA_MAX
    assert len(EC.CLAMPS_PROJECTED) == 2
    assert (EC.ROLL_PINHOLE.t_offset, EC.ROLL_EQUIRECT.t_offset) == (37.5, -40.0)


@pytest.mark.parametrize("case", EC.RADIAL, ids=ids)
def test_radial_cases_have_a_ray_without_angular_momentum(case):
    """The middle pixel of the odd frame looks along -pos, and the velocity, where there is one, lies along it too: in float32
    d x p is exactly 0 there, so m15L2 = 0 and Lv = 0, and the ray is a straight line into the hole."""
    w, h = case.size
    r32 = EC.reference(case, np.float32)
    p = EC.camera(case)["pos"].astype(np.float32)
    L = np.cross(r32["n"], p)
    assert L.dtype == np.float32
    radial = (L == 0).all(axis=2) & r32["inside"]
    print(f"[edges_ref] {case.name}: {int(radial.sum())} pixels with |d x p| == 0 in float32: {np.argwhere(radial).tolist()}")
    assert radial[h // 2, w // 2] and radial.sum() == 1
    assert r32["fate"][h // 2, w // 2] == 0 and r32["n_hits"][h // 2, w // 2] == 0      # captured, straight in
    if case.kind == P.FISHEYE:
        for dtype in (np.float32, np.float64):
            t = np.dtype(dtype).type
            x = ((np.arange(w, dtype=dtype) + t(0.5)) - t(w) / t(2)) * (t(2) / t(min(w, h)))
            y = (t(h) / t(2) - (np.arange(h, dtype=dtype) + t(0.5))) * (t(2) / t(min(w, h)))
            assert x[w // 2] == 0 and y[h // 2] == 0                  # rho == 0: inv = 0
            a, b, c, inside = P.pixel_coefficients(case.kind, case.fov, w, h, dtype)
            assert (a[h // 2, w // 2], b[h // 2, w // 2], c[h // 2, w // 2], inside[h // 2, w // 2]) == (1, 0, 0, True)


def test_clamp_cases_leave_the_clamped_range_on_the_sky():
    """observer_sky clamps D to [0.1, 1.5]: ahead of the fast camera rays that reach the sky have D above 1.5, beside the camera
    that flies sideways they have D below 0.1; the projected cases see both ends in one frame."""
    for case, low, high in ((EC.AHEAD_995, False, True), (EC.SIDEWAYS_995, True, False)) + tuple((c, True, True) for c in EC.CLAMPS_PROJECTED):
        for dtype in (np.float64, np.float32):
            r = EC.reference(case, dtype)
            D = r["D"][(r["fate"] == 1) & r["inside"]]
            print(f"[edges_ref] {case.name} {np.dtype(dtype).name}: D of the rays that reach the sky {D.min():.4f} .. {D.max():.3f}; "
                  f"{int((D < 0.1).sum())} under 0.1, {int((D > 1.5).sum())} over 1.5, {int(((D >= 0.1) & (D <= 1.5)).sum())} between")
            assert (D.min() < 0.1) == low and (D.max() > 1.5) == high
            assert ((D >= 0.1) & (D <= 1.5)).any()
        plain, shifted = EC.reference(case._replace(sky=False)), EC.reference(case)
        assert np.array_equal(plain["disk"], shifted["disk"]) and EC.rmse(plain["bg"], shifted["bg"]).max() > 1e-2
    D = np.concatenate([EC.reference(c)["D"].ravel() for c in EC.CLAMPS])
    assert D.min() < 0.1 and D.max() > 1.5


@pytest.mark.parametrize("case", EC.ROLL, ids=ids)
def test_the_roll_moves_the_disk_and_no_ray(case):
    still, rolled = EC.reference(case._replace(frame=0, speed=0.1)), EC.reference(case)
    moved = EC.rmse(still["disk"], rolled["disk"]).max()
    print(f"[edges_ref] {case.name}: t_offset {case.t_offset!r}; DISK moves by {moved:.3g} RMSE")
    assert moved > 0.1                                               # the device test asks its own two frames for 1e-2
    for k in ("fate", "n_hits", "steps", "D"):
        assert np.array_equal(still[k], rolled[k]), k
    assert abs(case.t_offset) <= 40.0                                # beyond, the float32 phi + t_offset Omega is the limit (below)


def test_the_float32_reference_is_over_the_cap_at_a_roll_of_300():
    """Why the roll cases stop at |t_offset| = 40 and look from (6, 0, 0.5): the float32 reference's phi + t_offset Omega loses
    the digits of phi that t_offset Omega takes, and at t_offset = 300 the float32 reference alone is off by more than 1e-3 on more
    pixels than the device is allowed.  Measured from (3, 2, 0.3) at tilt 25, 48 x 32, at rest: 0.20 % of the pixels at
    t_offset 0, 0.46 % at 40, 4.0 % at 300 (96 x 64: 0.26 %, 0.70 %, 4.2 %); the two roll cases are off on one pixel each
    (0.07 % and 0.05 %).  A bound on t_offset is the library's to set."""
    sky, tex = EC.scene()
    cam = EC.K.build_camera(list(EC.V1), 90.0, 48, 32, 10.0)
    share = {}
    for t_offset in (0.0, 300.0):
        a, b = (R.render(cam, (0.0, 0.0, 0.0), sky, tex, h_base=EC.STEP, tilt_deg=25.0, t_offset=t_offset, dtype=dt) for dt in (np.float64, np.float32))
        share[t_offset] = EC.off_share((a["bg"], a["disk"]), (b["bg"], b["disk"]))
    print(f"[edges_ref] share of pixels where the float32 reference is off by more than 1e-3, by t_offset: {share}")
    assert share[0.0] <= EC.OFF_SHARE < share[300.0]


def _without_late_crossings(case, dtype):
    """The frame of a case shaded with every crossing of rank 2 or more removed (the march is the same)."""
    march = R.march

    def two_at_most(*args, **kw):
        m = march(*args, **kw)
        m["hits"] = m["hits"][m["hits"][:, 1] < 2]
        return m
    R.march = two_at_most
    try:
        return EC.reference.__wrapped__(case, dtype)
    finally:
        R.march = march


@pytest.mark.parametrize("case", EC.CROSSINGS, ids=ids)
def test_many_crossing_cases_have_late_crossings_that_show(case):
    """At least 10 pixels whose ray crosses the disk three times or more -- the second crossing fills both parking slots, the
    march loop shades the oldest, and the third is parked in the slot that freed while the ray is still marching -- with equal
    fate and count in both dtypes, and on at least 5 of them the crossings after the second change DISK by more than 0.03: a
    flush that dropped them, or shaded them wrongly, shows."""
    r64, r32 = EC.reference(case, np.float64), EC.reference(case, np.float32)
    many = r64["n_hits"] >= 3
    assert np.array_equal(many, r32["n_hits"] >= 3)
    assert np.array_equal(r64["n_hits"][many], r32["n_hits"][many]) and np.array_equal(r64["fate"][many], r32["fate"][many])
    cut = _without_late_crossings(case, np.float64)
    assert cut["n_hits"].max() == r64["n_hits"].max() and np.array_equal(cut["disk"][~many], r64["disk"][~many])
    change = np.abs(cut["disk"] - r64["disk"]).max(axis=2)
    d32 = {k: float(np.abs(r32[k].astype(np.float64) - r64[k])[many].max()) for k in ("disk", "bg")}
    print(f"[edges_ref] {case.name}: {int(many.sum())} pixels with three or more crossings (at most {int(r64['n_hits'].max())}), "
          f"{int((many & (r64['fate'] == 1)).sum())} of them reach the sky; the crossings after the second change DISK by up to "
          f"{change.max():.3f}, by more than 0.03 on {int((change > 0.03).sum())} pixels; float32 against binary64 on them: {d32}")
    assert many.sum() >= 10
    assert (change[many] > 0.03).sum() >= 5
    assert (many & (r64["fate"] == 1)).sum() >= 10                   # what the device test's probe frame can count
