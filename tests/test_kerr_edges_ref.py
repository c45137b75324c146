"""The inputs of tests/test_gpu_kerr_edges.py are fair: on every case the float32 and the float64 run of the reference agree
on (nearly) every pixel's fate and crossing count, so the device test's cap on such pixels binds on the device alone; each frame
has both fates and disk light; and the conditions the device test leans on -- the roll moves the picture, a texture without
phi does not see it, the many-crossing views have many crossings, the mirror and up-down symmetries hold in the reference, the
refused cameras are refused -- are true of the reference.  No device."""
import numpy as np
import pytest

import kerr_cases as KC
import kerr_ref as K
from test_gpu_kerr import FATE_SHARE

COMPARED = KC.ROLL + list(KC.RINGS) + KC.VIEW_EDGES + KC.RAGGED + KC.CROSSINGS + [c for c in KC.UP_DOWN if c not in KC.VIEW_EDGES]


def _states(ref):
    """fate and crossing count of every pixel, as one array to compare."""
    return np.stack([ref["fate"].astype(np.int64), ref["n_hits"].astype(np.int64)], axis=-1)


@pytest.mark.parametrize("case", COMPARED, ids=lambda c: c.id)
def test_float32_and_float64_agree_on_fates_and_crossings(case):
    d32, share = KC.float32_distance(case)
    r64 = KC.edge_reference(case)
    print(f"{case.id}: float32 vs float64: fate / crossing count differs on {share:.3%}; distance {d32}")
    assert share <= FATE_SHARE / 4
    assert (r64["fate"] == 0).any() and (r64["fate"] == 1).any() and not (r64["fate"] == 2).any()
    assert r64["disk"].max() > 0 and r64["bg"].max() > 0
    assert all(np.isfinite(r64[k]).all() for k in ("bg", "disk", "final"))


def test_ragged_frames_keep_both_fates():
    small = KC.edge_reference(KC.RAGGED[3])
    assert (small["fate"].shape, int((small["fate"] == 0).sum()), int((small["fate"] == 1).sum())) == ((3, 5), 7, 8)
    assert int((small["disk"].max(axis=2) > 0).sum()) == 9


@pytest.mark.parametrize("case", KC.ROLL, ids=lambda c: c.id)
def test_the_roll_moves_the_disk(case):
    still, rolled = KC.edge_reference(case._replace(frame=0, speed=0.1)), KC.edge_reference(case)
    moved = KC.rmse(still["disk"], rolled["disk"])
    turns = case.t_offset * float(K.omega_kerr(np.float64(case.r_inner), case.A * K.M)) / (2 * np.pi)
    print(f"{case.id}: t_offset {case.t_offset!r}; DISK moves by {moved:.3g} RMSE; {turns:.1f} turns at the inner edge")
    assert moved > 0.1                                               # the device test asks its own two frames for 1e-2
    assert np.array_equal(_states(still), _states(rolled)) and np.array_equal(still["steps"], rolled["steps"])
    assert case.t_offset == pytest.approx({73: 7.3, 400: -40.0, 3000: 300.0}[case.frame], rel=1e-7)
    assert {73: 0 < turns < 1, 400: turns < -1, 3000: turns > 10}[case.frame]       # no wrap, the negative loop, many turns


def test_a_texture_without_phi_does_not_see_the_roll():
    """What the float32 reference's two frames differ by is the rounding of a bilinear sum of equal texels: the weights
    (1 - fu) and fu change with the roll, the texels they weigh do not.  A sum of four products of three factors is within 6
    ulp of the texel (at most 1); the opacity 1 - (1 - alpha)^6 multiplies an error of alpha by at most 6 and the brightness
    of a crossing stays under 3, so a layer moves by less than 6 * 6 * 3 * 2^-24 = 6.5e-6: asserted as 1e-5."""
    still, rolled = (KC.edge_reference(c, np.float32) for c in KC.RINGS)
    d = max(float(np.abs(still[k].astype(np.float64) - rolled[k]).max()) for k in ("bg", "disk"))
    print(f"float32 reference, rings texture, t_offset 0 against {KC.RINGS[1].t_offset}: largest difference {d:.3g}")
    assert d <= 1e-5
    assert np.array_equal(_states(still), _states(rolled))
    tex = KC.ring_disk()
    assert (tex == tex[:, :1]).all() and np.ptp(tex[:, 0, :3], axis=0).min() > 0.5 and np.ptp(tex[:, 0, 3]) > 0.2
    # ... and the same two frames under the project's own texture differ like any rolled pair
    assert KC.rmse(KC.edge_reference(KC.ROLL[0]._replace(frame=0))["disk"], KC.edge_reference(KC.ROLL[0])["disk"]) > 0.1


@pytest.mark.parametrize("case", KC.CROSSINGS, ids=lambda c: c.id)
def test_many_crossings(case):
    n = KC.edge_reference(case)["n_hits"]
    print(f"{case.id}: {int((n >= 3).sum())} pixels with three or more crossings, at most {int(n.max())}")
    assert (n >= 3).sum() >= 40


@pytest.mark.parametrize("A,view", KC.MIRRORS, ids=lambda v: str(v))
def test_a_hole_of_the_opposite_spin_is_the_mirror_image(A, view):
    """The reflection y -> -y with a -> -a maps the metric onto itself: the frame of (-A, (x, -y, z)) is the left-right flip
    (top-bottom from the pole, where the camera's right is x) -- of fates and crossings; the textures are not symmetric."""
    here = _states(KC.edge_reference(KC.Edge(A, view)))
    there = _states(KC.edge_reference(KC.Edge(-A, (view[0], -view[1], view[2]))))
    flipped = there[::-1] if view[0] == 0 and view[1] == 0 else there[:, ::-1]
    assert float((here != flipped).any(axis=-1).mean()) <= FATE_SHARE / 4
    if view[0] == 0 and view[1] == 0:
        assert np.array_equal(there[::-1], there[:, ::-1])          # on the axis either flip will do: the device test flips left-right
    else:
        own = float((here != here[:, ::-1]).any(axis=-1).mean())
        print(f"A={A} {view}: {own:.1%} of the pixels differ from the frame's own flip")
        assert own > 0.3


@pytest.mark.parametrize("case", KC.UP_DOWN, ids=lambda c: c.id)
def test_the_equatorial_view_is_its_own_top_bottom_flip(case):
    assert case.view[2] == 0.0 and case.height % 2 == 0              # no ray lies in the plane
    for dtype in (np.float64, np.float32):
        ref = KC.edge_reference(case, dtype)
        assert np.array_equal(_states(ref), _states(ref)[::-1])
        asym = KC.rmse(ref["disk"], ref["disk"][::-1])
        print(f"{case.id} {np.dtype(dtype).name}: DISK against its top-bottom flip {asym:.3g}")
        assert asym <= 1e-5
    assert KC.rmse(ref["bg"], ref["bg"][::-1]) > 1e-2                # the sky is not symmetric: the device test flips the probe's


def test_the_camera_stays_outside_the_static_limit():
    sky, tex = KC.scene()
    for A, view in KC.INSIDE_STATIC_LIMIT:
        f, r = K.camera_f(view, A)
        assert f >= 1.0
        for render in (K.render, __import__("kerr_redshift_ref").render):
            with pytest.raises(ValueError, match="static limit"):
                render(K.build_camera(list(view), KC.FOV, 8, 8, KC.R_MAX), A, sky, tex)
    assert K.camera_f(KC.INSIDE_STATIC_LIMIT[1][1], 0.998)[1] < K.r_plus(0.998)
    f, r = K.camera_f(KC.CLOSE_IN.view, KC.CLOSE_IN.A)
    print(f"close in: f = {f:.4f} at r = {r:.4f}")
    assert 0.75 < f < 1.0                                              # just outside: the case renders
    # inside the horizon f may fall under 1 again (towards the ring): refused all the same
    with pytest.raises(ValueError, match="static limit"):
        K.check_camera((0.3, 0.2, 0.1), 0.998)
    assert K.camera_f((0.3, 0.2, 0.1), 0.998)[0] < 1.0
    # the package's own statement of the rule (the command line's refusal) is the reference's
    from bhr_amd import kerr
    for A, view in KC.INSIDE_STATIC_LIMIT + ((KC.CLOSE_IN.A, KC.CLOSE_IN.view), (0.998, (0.3, 0.2, 0.1)), (-0.6, (6.0, 0.0, 0.5)), (0.0, (0.999, 0.0, 0.0))):
        assert kerr.camera_f(view, A) == pytest.approx(K.camera_f(view, A), rel=1e-14)
        try:
            K.check_camera(view, A)
            inside = False
        except ValueError:
            inside = True
        assert kerr.camera_outside_static_limit(view, A) == (not inside)
    K.check_camera((6.0, 0.0, 0.5), 0.998)
    K.check_camera((1.001, 0.0, 0.0), 0.0)
    with pytest.raises(ValueError, match="static limit"):
        K.check_camera((0.999, 0.0, 0.0), 0.0)
