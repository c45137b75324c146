"""Kerr point stars on the CPU: the point stars' model (tests/stars_ref.py, include/bhr.h "point stars") read over the escape
directions of the Kerr march (tests/kerr_ref.py), and the new entry points' names.  No GPU.

The model is agnostic of the metric: it takes a status plane, a plane of escape directions and the camera-side pixel directions.
What this file checks is that the Kerr map's planes are a sound input to it -- the critical curve of a spinning hole is
asymmetric and its caustic is not a point, so the folds and the squeezed triangles lie elsewhere than in the Schwarzschild
tests -- by the same measure the device tests use: the float32 evaluation of the reference against the binary64 one on the same
float32 planes, share of the pixels beyond 1e-3 of the maximum at most 0.5 % (the device tests' cap; stars_ref.outlier_share).
On those views the share is 0 and the distance between 2e-8 and 1e-7, so the cap is one the reference alone meets.

kerr_ref.march in float32 gives what the device's map holds: float32 escape directions, normalized by the march itself, zeroed
here where the ray did not escape (the build kernel stores zeros there)."""
import functools

import numpy as np
import pytest

import kerr_ref as K
import stars_ref as R

FOV, STEP = 90.0, 0.1
# (view, spin, width, height)
CASES = {
    "far_prograde": ((6.0, 0.0, 0.5), 0.9, 96, 64),
    "far_retrograde": ((6.0, 0.0, 0.5), -0.9, 96, 64),
    "near_extreme": ((3.0, 2.0, 0.3), 0.998, 96, 64),
    "pole": ((1.0, 0.0, 6.0), 0.9, 96, 64),
    "ragged_61x43": ((6.0, 0.0, 0.5), 0.9, 61, 43),
    "ragged_31x17": ((3.0, 2.0, 0.3), 0.6, 31, 17),
}


@functools.lru_cache(maxsize=None)
def _tables():
    from bhr_amd import skybox
    return skybox.sky_tables(2048, 1024, 42, 6000)


def kerr_planes(cam, A):
    """(status (H, W) int32, escape_dir (H, W, 3) float32) of the float32 Kerr march of the camera's view."""
    H, W = cam["height"], cam["width"]
    d = K.pixel_rays(cam, np.float32).reshape(-1, 3)
    m = K.march(cam["pos"], d, A, h_base=STEP, r_escape=float(cam["r_escape"]), dtype=np.float32)
    esc = m["esc_dir"].astype(np.float32)
    esc[m["fate"] != 1] = 0.0
    return m["fate"].astype(np.int32).reshape(H, W), esc.reshape(H, W, 3)


@pytest.mark.parametrize("case", list(CASES))
def test_float32_reference_meets_the_device_cap_over_kerr_planes(case):
    from bhr_amd import stars
    pos, A, W, H = CASES[case]
    cam = K.build_camera(list(pos), FOV, W, H)
    status, esc = kerr_planes(cam, A)
    dirs, flux = stars.catalog_from_tables(_tables(), 2.0, float(cam["pw"]) * float(cam["ph"]))
    d = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    f = flux.astype(np.float32)
    S64 = R.star_plane(status, esc, K.pixel_rays(cam, np.float64), d, f)
    S32 = R.star_plane(status, esc, K.pixel_rays(cam, np.float32), d, f, dtype=np.float32)
    share, dist = R.outlier_share(S32, S64), R.distance(S32, S64)
    print(f"{case}: A = {A}, {W} x {H}: escaped {int((status == 1).sum())} of {W * H}, lit pixels {int(S64.any(axis=-1).sum())}, "
          f"share beyond 1e-3 of the maximum {share:.5f}, distance {dist:.3e}")
    assert (status == 1).any() and (status == 0).any(), "the view shows no shadow"
    assert S64.max() > 0 and np.isfinite(S32).all() and (S32 >= 0).all()
    assert share <= 0.005, f"{case}: {share:.4%} of the pixels beyond 1e-3 of the maximum"


def test_entry_points_are_declared_and_exported(hip_lib):
    from bhr_amd import HipRenderer, _lib
    for name in ("bhr_set_kerr_stars", "bhr_get_kerr_stars_info", "bhr_kerr_stars_resources"):
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name), name
    for name in ("set_kerr_stars", "clear_kerr_stars", "kerr_stars_info", "read_kerr_star_plane", "kerr_stars_resources"):
        assert callable(getattr(HipRenderer, name)), name
