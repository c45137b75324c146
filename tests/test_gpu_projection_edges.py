"""The projections on the device beyond the frames of tests/test_gpu_projection.py: ragged and tiny panoramas and domes with a
moving camera, a 10 x 5 degree panorama and a 10 degree dome, a 360 degree dome over a tilted disk, a tall dome, the camera on
the pole, 0.995 ahead and sideways, the dome's rho == 0 pixel (inv = 0, an exactly radial ray); a rolled disk (t_offset); rays
with three and more disk crossings (parked in a slot the projected object's in-loop flush freed); supersampling at 4 and 8 of a dome whose fine
frame is odd x k; and the sky's clamps apart from the march.  tests/test_observer_edges_ref.py shows, without a device, that the
inputs are fair.

Bars: tests/test_gpu_observer.py's, as they are (tests/observer_edge_cases.py: check_frame_bars states them once for this file and
tests/test_gpu_observer_edges.py); a dome's pixels outside the float32 reference's mask are exactly 0 in BG and DISK."""
import pytest

import observer_edge_cases as EC
import projection_ref as P
from test_gpu_projection import BAR_FLOOR, OFF_SHARE, STEPS_RTOL

pytestmark = pytest.mark.gpu

TAG = "projection edges"
ids = lambda c: c.name
SUPERSAMPLED = EC.Edge("ss_fish180_9x9", EC.V1, EC.MOVING, kind=P.FISHEYE, fov=EC.FISH_180, size=(9, 9), tilt=25.0)


def test_the_bars_are_the_projection_tests():
    assert (EC.BAR_FLOOR, EC.OFF_SHARE, EC.STEPS_RTOL) == (BAR_FLOOR, OFF_SHARE, STEPS_RTOL)


@pytest.mark.parametrize("case", EC.PROJECTIONS, ids=ids)
def test_projections_against_the_reference(case, hip_lib):
    got = EC.check_against_reference(case, TAG)
    assert got["steps"] > 0 and got["bg"].max() > 0 and got["disk"].max() > 0


def test_rays_with_three_and_more_crossings(hip_lib):
    EC.check_many_crossings(EC.CROSSINGS_EQUIRECT, TAG)


def test_rolled_disk_against_the_reference(hip_lib):
    EC.check_roll(EC.ROLL_EQUIRECT, TAG)


@pytest.mark.parametrize("k", (4, 8))
def test_supersampled_dome_is_the_box_filter_of_the_fine_frame(k, hip_lib):
    """The rim's zeros enter the filter, and the fine frame is odd x k (36 x 36, 72 x 72): its centre lies on a pixel corner."""
    ss, fine = EC.check_supersampled(SUPERSAMPLED, k, TAG)
    blank = (fine["bg"] == 0).all(axis=2) & (fine["disk"] == 0).all(axis=2)
    assert blank[0, 0] and blank[-1, -1] and not blank.all()


@pytest.mark.parametrize("case", EC.CLAMPS_PROJECTED, ids=ids)
def test_sky_clamps(case, hip_lib):
    EC.check_sky_clamps(case, TAG)
