"""The moving observer on the device beyond the two views of tests/test_gpu_observer.py: cameras on the pole, in the disk's plane,
below it, close in, far out and wide; velocities of 0.995 ahead and sideways, where D leaves the sky's clamp at either end, and
0.6 directly away; ragged and tiny frames with a moving camera, one of them with an exactly radial ray; a rolled disk (t_offset);
rays with three and more disk crossings (a crossing parked in a slot that ObserverRay::flush_one freed inside the march loop, and
shaded with the lane's D behind two others); supersampling at 4 and 8; and the sky's clamps apart from the march.  tests/test_observer_edges_ref.py shows, without a device, that the inputs are fair.

Bars: tests/test_gpu_observer.py's, as they are (tests/observer_edge_cases.py: check_frame_bars states them once for this file and
tests/test_gpu_projection_edges.py).  Per layer and channel the device is allowed twice the distance the float32 run of
observer_ref keeps from its binary64 run on the same case, never less than 1e-4; at most 0.5 % of the pixels (one pixel of a frame
of fewer than 200) may be off by more than 1e-3; the step total stays within 2e-4 of the float32 reference's, never held tighter
than 2 steps."""
import pytest

import observer_edge_cases as EC
from test_gpu_observer import BAR_FLOOR, OFF_SHARE, STEPS_RTOL

pytestmark = pytest.mark.gpu

TAG = "observer edges"
ids = lambda c: c.name
SUPERSAMPLED = tuple(EC.Edge(f"ss_{w}x{h}", EC.V1, EC.MOVING, size=(w, h), tilt=25.0) for w, h in ((12, 8), (7, 5)))


def test_the_bars_are_the_observer_tests():
    assert (EC.BAR_FLOOR, EC.OFF_SHARE, EC.STEPS_RTOL) == (BAR_FLOOR, OFF_SHARE, STEPS_RTOL)


@pytest.mark.parametrize("case", EC.VIEW_EDGES, ids=ids)
def test_views_against_the_reference(case, hip_lib):
    EC.check_against_reference(case, TAG)


@pytest.mark.parametrize("case", EC.VELOCITIES, ids=ids)
def test_velocities_against_the_reference(case, hip_lib):
    EC.check_against_reference(case, TAG)


@pytest.mark.parametrize("case", EC.RAGGED, ids=ids)
def test_ragged_and_tiny_frames_against_the_reference(case, hip_lib):
    got = EC.check_against_reference(case, TAG)
    assert got["steps"] > 0 and got["bg"].max() > 0 and got["disk"].max() > 0


def test_rays_with_three_and_more_crossings(hip_lib):
    EC.check_many_crossings(EC.CROSSINGS_PINHOLE, TAG)


def test_rolled_disk_against_the_reference(hip_lib):
    EC.check_roll(EC.ROLL_PINHOLE, TAG)


@pytest.mark.parametrize("k", (4, 8))
@pytest.mark.parametrize("case", SUPERSAMPLED, ids=ids)
def test_supersampled_frames_are_the_box_filter_of_the_fine_frame(case, k, hip_lib):
    """The resolve is a butterfly over the wave: k = 4 and 8 use other lane strides than k = 2, at k = 8 one output pixel is a
    whole tile, and a fine frame that is no multiple of 8 (28 x 20, 56 x 40) has lanes beyond the edge inside a k x k group."""
    EC.check_supersampled(case, k, TAG)


@pytest.mark.parametrize("case", EC.CLAMPS, ids=ids)
def test_sky_clamps(case, hip_lib):
    EC.check_sky_clamps(case, TAG)
