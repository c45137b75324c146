"""The frames the observer tests share: the cases of the device test and their observer_ref frames, each computed once."""
import functools
import typing

import numpy as np

import kerr_ref as K
import observer_ref as R

W, H, FOV, STEP = 96, 64, 90.0, 0.1
R_INNER, R_OUTER, R_MAX = 2.0, 15.0, 10.0
VIEWS = ((6.0, 0.0, 0.5), (3.0, 2.0, 0.3))
TILTS = (0.0, 25.0)


class Case(typing.NamedTuple):
    name: str
    view: tuple
    beta: tuple
    tilt: float = 0.0
    sky: bool = True


def _forward(view, speed):
    p = np.array(view, dtype=np.float64)
    return tuple(float(v) for v in -speed * p / np.linalg.norm(p))


def _named(kind, view):
    return tuple(float(v) for v in R.velocity(kind, view))


# the device test's cases: the two named velocities, a general one, a fast one dead ahead, a tilted disk, a plain sky
CASES = (Case("circular", VIEWS[0], _named("circular", VIEWS[0])),
         Case("infall", VIEWS[0], _named("infall", VIEWS[0])),
         Case("general", VIEWS[1], (0.3, -0.4, 0.5)),
         Case("forward_0.9", VIEWS[0], _forward(VIEWS[0], 0.9)),
         Case("circular_tilt25", VIEWS[1], _named("circular", VIEWS[1]), tilt=25.0),
         Case("infall_plain_sky", VIEWS[1], _named("infall", VIEWS[1]), sky=False))
AT_REST = tuple(Case(f"rest_{v[0]:g}_tilt{t:g}", v, (0.0, 0.0, 0.0), tilt=t) for v in VIEWS for t in TILTS)


@functools.lru_cache(maxsize=None)
def scene():
    from bhr_amd import scenes
    return scenes.analytic_skybox(), scenes.noisy_disk()


def camera(view, width=W, height=H):
    return K.build_camera(list(view), FOV, width, height, R_MAX)


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64, width=W, height=H):
    """observer_ref's frame of a case (read-only: shared between tests)."""
    sky, tex = scene()
    out = R.render(camera(case.view, width, height), case.beta, sky, tex, h_base=STEP, r_inner=R_INNER, r_outer=R_OUTER,
                   tilt_deg=case.tilt, sky_shift_on=case.sky, dtype=dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


def rmse(a, b):
    """Per-channel RMSE of two (H, W, 3) layers."""
    return np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2, axis=(0, 1)))


def off_share(a, b, tol=1e-3):
    """Share of the pixels that differ by more than tol in any channel of any of the layer pairs (a[k], b[k])."""
    bad = np.zeros(a[0].shape[:2], dtype=bool)
    for x, y in zip(a, b):
        bad |= (np.abs(np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)) > tol).any(axis=2)
    return float(bad.mean())
