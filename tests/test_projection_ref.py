"""tests/projection_ref.py, the CPU reference of the projections, checked against the geometry it states and in float32 against
binary64 on the device test's cases (no GPU; the product is used for the shared scene only)."""
import numpy as np
import pytest

import projection_cases as PC
import projection_ref as P

BAR_FLOOR = 1e-4            # tests/test_gpu_projection.py's bars
OFF_SHARE = 0.005
STEPS_RTOL = 2e-4


def _cam(size, view=PC.V0):
    return PC.camera(view, *size)


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("binary64", "float32"))
def test_directions_are_unit(case, dtype):
    n, inside = P.directions(_cam(case.size, case.view), case.kind, case.fov, dtype)
    assert n.dtype == dtype and n.shape == (case.size[1], case.size[0], 3)
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1.0).max() <= 1e-6     # masked pixels included: they are built like any other


def test_equirect_looks_where_it_says():
    W, H = 64, 32
    cam = _cam((W, H))
    F, R, U = (cam[k].astype(np.float64) for k in ("forward", "right", "up"))
    n, inside = P.directions(cam, P.EQUIRECT, (360.0, 180.0))
    assert inside.all()
    centre = n[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].mean(axis=(0, 1))         # the four pixels around the image centre
    assert np.allclose(centre / np.linalg.norm(centre), F, atol=1e-6)
    # lon = +-90 degrees lies on the pixel boundaries i = 3 W / 4 and W / 4: the two pixels astride them average to +-R
    for i, want in ((3 * W // 4, R), (W // 4, -R)):
        m = n[H // 2 - 1:H // 2 + 1, i - 1:i + 1].mean(axis=(0, 1))
        assert np.allclose(m / np.linalg.norm(m), want, atol=1e-6)
    # the top row looks towards up, the bottom row away from it: lat = +-90 (1 - 1 / H) degrees
    assert np.allclose(n[0] @ U, np.sin(np.radians(90.0 * (1 - 1 / H)))) and np.allclose(n[-1] @ U, -np.sin(np.radians(90.0 * (1 - 1 / H))))
    assert (np.diff(n[H // 2] @ R)[W // 4:3 * W // 4 - 1] > 0).all()                     # longitude grows towards right
    # a partial panorama is the middle of the full one
    part, _ = P.directions(cam, P.EQUIRECT, (180.0, 90.0))
    assert np.allclose(part[0, 0] @ U, np.sin(np.radians(45.0 * (1 - 1 / H)))) and part[0, 0] @ R < 0 < part[0, -1] @ R


@pytest.mark.parametrize("fov", (180.0, 360.0, 90.0))
@pytest.mark.parametrize("size", ((64, 64), (64, 48), (33, 47)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_fisheye_looks_where_it_says(size, fov):
    W, H = size
    cam = _cam(size)
    F, R, U = (cam[k].astype(np.float64) for k in ("forward", "right", "up"))
    n, inside = P.directions(cam, P.FISHEYE, (fov,))
    a, b, c, _ = P.pixel_coefficients(P.FISHEYE, (fov,), W, H)
    m = min(W, H)
    x = (np.arange(W) + 0.5 - W / 2)[None, :] * (2.0 / m)
    y = (H / 2 - (np.arange(H) + 0.5))[:, None] * (2.0 / m)
    rho = np.sqrt(x * x + y * y)
    # equidistant: the angle from forward is rho fov / 2 -- fov / 2 on the rim -- and the azimuth is the pixel's own (the
    # camera's basis is float32: orthonormal to 1e-7)
    assert np.allclose((n @ F)[inside], np.cos(rho * np.radians(fov) / 2)[inside], atol=1e-6)
    assert np.allclose(np.linalg.norm(np.cross(n, F), axis=-1)[inside], np.abs(np.sin(rho * np.radians(fov) / 2))[inside], atol=1e-6)
    assert np.array_equal(inside, rho <= 1.0)
    off_axis = inside & (np.sin(rho * np.radians(fov) / 2) > 1e-3)        # where the azimuth is defined (not at the centre, nor at a 360 degree rim)
    st = np.sin(rho * np.radians(fov) / 2)[off_axis]
    assert np.allclose((n @ R)[off_axis] / st, np.broadcast_to(x, rho.shape)[off_axis] / rho[off_axis], atol=1e-4)
    assert np.allclose((n @ U)[off_axis] / st, np.broadcast_to(y, rho.shape)[off_axis] / rho[off_axis], atol=1e-4)
    # the image circle covers pi / 4 of the inscribing square, to within the pixels its rim passes through
    rim = int(((rho > 1.0 - np.sqrt(2.0) / m) & (rho < 1.0 + np.sqrt(2.0) / m)).sum())
    assert abs(int(inside.sum()) - np.pi / 4 * m * m) <= rim
    if W == H and W % 2 == 0:
        centre = n[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].mean(axis=(0, 1))
        assert np.allclose(centre / np.linalg.norm(centre), F, atol=1e-6)


def test_fisheye_centre_pixel_is_forward():
    """rho = 0 (an odd frame's middle pixel): inv = 0, and the direction is forward itself."""
    for dtype in (np.float64, np.float32):
        cam = _cam((5, 5))
        n, inside = P.directions(cam, P.FISHEYE, (180.0,), dtype)
        assert inside[2, 2] and np.array_equal(n[2, 2], cam["forward"].astype(dtype))
        one, ins = P.directions(_cam((1, 1)), P.FISHEYE, (180.0,), dtype)
        assert ins.all() and np.array_equal(one[0, 0], cam["forward"].astype(dtype))


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.name)
def test_float32_mask_is_the_binary64_mask(case):
    _, m32 = P.directions(_cam(case.size, case.view), case.kind, case.fov, np.float32)
    _, m64 = P.directions(_cam(case.size, case.view), case.kind, case.fov, np.float64)
    assert np.array_equal(m32, m64)
    assert m64.all() == (case.kind == P.EQUIRECT)


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.name)
def test_float32_reference_is_within_the_device_bars(case):
    r64, r32 = PC.reference(case, np.float64), PC.reference(case, np.float32)
    share = PC.off_share((r32["bg"], r32["disk"]), (r64["bg"], r64["disk"]))
    s32, s64 = int(r32["steps"].sum()), int(r64["steps"].sum())
    print(f"[projection_ref] {case.name}: off share {share:.2e}, RMSE bg {PC.rmse(r32['bg'], r64['bg']).max():.1e} disk "
          f"{PC.rmse(r32['disk'], r64['disk']).max():.1e}, steps f32 {s32} binary64 {s64}")
    assert share <= OFF_SHARE
    assert abs(s32 - s64) <= STEPS_RTOL * s64
    for layer in ("bg", "disk"):
        assert (PC.rmse(r32[layer], r64[layer]) <= BAR_FLOOR).all()
        assert np.isfinite(r32[layer]).all()
    off = ~r64["inside"]
    for r in (r64, r32):                                   # a masked pixel: exactly 0, no step
        assert (r["bg"][off] == 0).all() and (r["disk"][off] == 0).all() and (r["steps"][off] == 0).all()
    assert r64["disk"].max() > 0 and r64["bg"].max() > 0 and (r64["steps"][r64["inside"]] > 0).all()


def test_null_observer_is_at_rest_with_a_plain_sky():
    case = PC.AT_REST[3]
    sky, tex = PC.scene()
    cam = _cam((24, 24))
    a = P.render(cam, case.kind, case.fov, None, sky, tex)
    for shift in (False, True):                            # D = 1 at rest: the shifted sky is the plain one
        b = P.render(cam, case.kind, case.fov, (0.0, 0.0, 0.0), sky, tex, sky_shift_on=shift)
        assert all(np.array_equal(a[k], b[k]) for k in ("bg", "disk", "steps"))
    moving = P.render(cam, case.kind, case.fov, (0.0, 0.5, 0.0), sky, tex)
    assert not np.array_equal(moving["bg"], a["bg"]) and np.array_equal(moving["inside"], a["inside"])
