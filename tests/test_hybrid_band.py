"""The binary64 restatement of the hybrid classification (tests/hybrid_band.py) against the CPU oracle's own rays: its
pixel geometry (row direction, half-pixel offsets, the global row) and its first-integral impact parameter b must predict
which rays the oracle's march captures.  Without this the GPU checks of tests/test_gpu_hybrid_band.py could hold the
library's tiles against the wrong pixels.  No GPU."""
import numpy as np
import pytest

import hybrid_band as hb

W, H = 128, 72
# r0 in {1.3, 2, 2.6, 4, 6, 30}: inside the photon sphere, inside 3 r_s (b and b_l differ by up to 17 % there), the
# default pov, a telephoto far camera; slightly off the disk plane, off the x axis.  (cam, fov, look_away_deg): the views
# turned away from the hole hold outgoing rays, which a look-at camera never has; the pitched ones put the hole's image
# off the middle row, so that the row direction matters.  (cam, fov, look_away_deg, pitch_deg)
VIEWS = [([1.3, 0.0, 0.05], 120.0, 110.0, 0.0), ([1.9, 0.5, 0.3], 160.0, 0.0, 0.0), ([2.0, 0.4, 0.3], 100.0, 80.0, 0.0),
         ([2.0, -0.4, 0.3], 110.0, 0.0, 70.0), ([2.6, 0.3, 0.2], 150.0, 0.0, 0.0), ([2.6, 0.3, 0.2], 100.0, 60.0, 0.0),
         ([3.6, -1.5, 0.8], 100.0, 0.0, 0.0), ([6.0, 0.0, 0.5], 90.0, 0.0, 20.0), ([6.0, 0.0, 0.5], 90.0, 0.0, 0.0),
         ([29.0, 7.0, 3.0], 20.0, 0.0, -4.0)]
KEEP_OUT = 0.02           # |b - b_c| below this: the march's own step error decides


def oracle_escapes(oracle, cam, fov, look, pitch):
    """(H, W) bool: the oracle's march of these rays escapes (a transparent disk: nothing but the hole stops a ray)."""
    ora = oracle.OracleRenderer(W, H, np.ones((16, 32, 3), np.float32), np.zeros((8, 32, 4), np.float32), step_size=0.1,
                                r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0)
    if look or pitch:                                         # the oracle's march from the turned camera's uniforms
        u = ora.camera_uniforms(cam, fov)
        c = hb.uniforms(cam, fov, W, H, look, pitch)
        u.cam_forward[:], u.cam_right[:], u.cam_up[:] = list(c.forward), list(c.right), list(c.up)
        ora.camera_uniforms = lambda *_: u
    return np.abs(ora.escape_directions(cam, fov)).sum(axis=2).T > 0


@pytest.mark.parametrize("cam_pos,fov,look,pitch", VIEWS, ids=[f"r{np.linalg.norm(v[0]):.1f}-look{v[2]:.0f}-pitch{v[3]:.0f}" for v in VIEWS])
def test_helper_b_predicts_the_oracle_s_captures(cam_pos, fov, look, pitch, oracle):
    """Outside the photon sphere a ray is captured iff it is ingoing with b < b_c; inside it, it escapes iff it is
    outgoing with b < b_c."""
    escaped = oracle_escapes(oracle, cam_pos, fov, look, pitch)
    geo = hb.pixel_geometry(hb.uniforms(cam_pos, fov, W, H, look, pitch), W, H, 0, H)
    r0 = float(np.sqrt(geo["r0sq"]))
    b, out = geo["b"], geo["cos_out"] > 0
    inner = b < hb.B_CRIT
    want_escaped = (out & inner) if r0 < 1.5 else ~(~out & inner)
    sure = np.abs(b - hb.B_CRIT) > KEEP_OUT
    assert sure.sum() > 0.8 * W * H, (r0, int(sure.sum()))
    assert want_escaped[sure].any() and not want_escaped[sure].all(), "the view must show both fates"
    assert out.any() == (abs(look) + abs(pitch) + fov / 2 > 90), "outgoing rays: the views turned beyond the field's edge only"
    bad = sure & (escaped != want_escaped)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        pytest.fail(f"r0 {r0:.2f}: {int(bad.sum())} pixels disagree; first ({x}, {y}): b - b_c {b[y, x] - hb.B_CRIT:+.4f}, "
                    f"outgoing {bool(out[y, x])}, oracle escaped {bool(escaped[y, x])}")
    # b_l (the local moment) is NOT the orbit's invariant near the hole: it would misplace the ring
    if r0 < 3:
        assert np.abs(geo["b"] / geo["b_l"] - 1).max() > 0.05


def test_helper_pixel_rows_are_global():
    """A row block's pixel geometry is the whole frame's at the same global rows."""
    cam = hb.uniforms([6.0, 0.0, 0.5], 90.0, W, H)
    full = hb.pixel_geometry(cam, W, H, 0, H)
    part = hb.pixel_geometry(cam, W, H, 21, 53)
    np.testing.assert_array_equal(part["b"], full["b"][21:53])
    # the look-at camera's centre is the hole: the four centre pixels lie half a pixel's diagonal off it (b ~ 0.12 here)
    assert full["b"][H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].max() < 0.15


def test_tile_flags_cover_the_band_at_a_small_view():
    """The restated rule keeps its own promise on a small view (the GPU test holds the library to both)."""
    for cam_pos, fov, look, pitch in VIEWS:
        cam = hb.uniforms(cam_pos, fov, W, H, look, pitch)
        lo, hi = hb.effective_band(0.1)
        flags, margin, _ = hb.tile_flags(cam, W, H, 0, H, 0.0, lo, hi)
        need = hb.must_be_strict(hb.pixel_geometry(cam, W, H, 0, H), lo, hi)
        tiles = hb.tile_of_pixels(W, 0, 0, H)
        assert not (need & ~flags.ravel()[tiles]).any(), cam_pos
        assert flags.any(), cam_pos


def test_effective_band_widens_beyond_step_0_1():
    assert hb.effective_band(0.05) == (hb.BAND_LO, hb.BAND_HI)
    assert hb.effective_band(0.1) == (hb.BAND_LO, hb.BAND_HI)
    lo, hi = hb.effective_band(0.3)
    assert abs(lo / hb.BAND_LO - 3) < 1e-6 and abs(hi / hb.BAND_HI - 3) < 1e-6
