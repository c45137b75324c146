"""The frames the projection tests share: the cases of the device test and their projection_ref frames, each computed once."""
import functools
import typing

import numpy as np

import kerr_ref as K
import observer_cases as OC
import observer_ref as R
import projection_ref as P

STEP, R_INNER, R_OUTER, R_MAX = 0.1, 2.0, 15.0, 10.0


class Case(typing.NamedTuple):
    name: str
    view: tuple
    kind: str
    fov: tuple
    size: tuple
    tilt: float = 0.0
    beta: typing.Optional[tuple] = None          # None: the camera stands still (obs = NULL)
    sky: bool = True


V0, V1 = OC.VIEWS                                # (6, 0, 0.5) and (3, 2, 0.3)
FORWARD_09 = tuple(float(v) for v in -0.9 * np.array(V0) / np.linalg.norm(np.array(V0)))

AT_REST = (Case("eq_full", V0, P.EQUIRECT, (360.0, 180.0), (96, 48)),
           Case("eq_full_close_tilt", V1, P.EQUIRECT, (360.0, 180.0), (96, 48), tilt=25.0),
           Case("eq_part", V0, P.EQUIRECT, (120.0, 60.0), (96, 48)),
           Case("fish180", V0, P.FISHEYE, (180.0,), (64, 64)),
           Case("fish360_close_tilt", V1, P.FISHEYE, (360.0,), (64, 48), tilt=25.0))
MOVING = (Case("eq_full_circular", V0, P.EQUIRECT, (360.0, 180.0), (96, 48), beta=tuple(float(v) for v in R.velocity("circular", V0))),
          Case("fish180_forward", V0, P.FISHEYE, (180.0,), (64, 64), beta=FORWARD_09))
CASES = AT_REST + MOVING


def scene():
    return OC.scene()


def camera(view, width, height):
    """The camera's basis and position (its image plane is not used: any field of view)."""
    return K.build_camera(list(view), 90.0, width, height, R_MAX)


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64):
    """projection_ref's frame of a case (read-only: shared between tests)."""
    sky, tex = scene()
    out = P.render(camera(case.view, *case.size), case.kind, case.fov, case.beta, sky, tex, h_base=STEP, r_inner=R_INNER, r_outer=R_OUTER,
                   tilt_deg=case.tilt, sky_shift_on=case.sky, dtype=dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


rmse, off_share = OC.rmse, OC.off_share
