"""The frames the Kerr camera's tests share (tests/test_kerr_observer_ref.py on the CPU, tests/test_gpu_kerr_observer.py on the
device): the cases and their kerr_observer_ref frames, each computed once."""
import functools
import typing

import numpy as np

import kerr_cases as KC
import kerr_observer_ref as V
import kerr_ref as K


class Case(typing.NamedTuple):
    """One view of the Kerr camera.  `beta`: a velocity, or the name of one evaluated at `view` (kerr_observer_ref.velocity);
    None: the call without a velocity.  `projection`: None (the pinhole of `fov`), "equirect" or "fisheye" with `pfov`."""
    A: float
    view: tuple
    beta: typing.Union[None, str, tuple] = None
    sky: bool = True
    projection: typing.Optional[str] = None
    pfov: typing.Optional[tuple] = None
    redshift: str = "model"
    width: int = KC.W
    height: int = KC.H
    fov: float = KC.FOV
    force: bool = False          # the Kerr kernels at A = 0

    @property
    def id(self):
        b = "rest" if self.beta is None else self.beta if isinstance(self.beta, str) else "b" + "_".join(f"{v:g}" for v in self.beta)
        s = f"A{self.A:g}-pov{self.view[0]:g}_{self.view[1]:g}_{self.view[2]:g}-{b}-{self.redshift}-{self.width}x{self.height}"
        if self.projection:
            s += f"-{self.projection}" + "_".join(f"{v:g}" for v in self.pfov)
        return s + ("" if self.sky else "-plain")


def beta_of(case):
    """The velocity of a case as three float32 -- what the call carries -- or None."""
    if case.beta is None:
        return None
    b = V.velocity(case.beta, case.view, case.A) if isinstance(case.beta, str) else np.asarray(case.beta, dtype=np.float64)
    return tuple(float(v) for v in b.astype(np.float32))


# the issue's list: two named velocities, a free one under the exact redshift, the full sphere at rest, a moving fisheye wider than a
# hemisphere, and the plain sky
REFERENCE = (
    Case(0.9, (3.0, 2.0, 0.0), "circular"),
    Case(0.998, (3.0, 2.0, 0.3), "zamo"),
    Case(-0.9, (6.0, 0.0, 0.5), (0.3, -0.4, 0.5), redshift="exact"),
    Case(0.9, (6.0, 0.0, 0.5), None, projection="equirect", pfov=(360.0, 180.0), width=96, height=48),
    Case(0.6, (6.0, 0.0, 0.5), (0.2, 0.3, -0.1), projection="fisheye", pfov=(220.0,), width=64, height=64),
    Case(0.9, (3.0, 2.0, 0.0), "circular", sky=False, redshift="exact"),
)
# forced Kerr at A = 0 against the Schwarzschild observer and projected marches of the same view and velocity
SCHWARZSCHILD = (
    Case(0.0, (6.0, 0.0, 0.5), (0.3, -0.4, 0.5), force=True),
    Case(0.0, (3.0, 2.0, 0.3), (0.2, 0.3, -0.1), projection="fisheye", pfov=(180.0,), width=64, height=64, force=True),
)


def camera(case):
    return K.build_camera(list(case.view), 90.0 if case.projection else case.fov, case.width, case.height, KC.R_MAX)


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64):
    """kerr_observer_ref's frame of a case (read-only: shared between tests)."""
    sky, tex = KC.scene()
    out = V.render(camera(case), case.A, sky, tex, beta=beta_of(case), sky_shift_on=case.sky, projection=case.projection, fov=case.pfov,
                   redshift=case.redshift, h_base=KC.STEP, r_inner=KC.R_INNER, r_outer=KC.R_OUTER, dtype=dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


def float32_distance(case):
    """kerr_cases.float32_distance for a Case: (per-layer distance of the float32 run from the binary64 one over the pixels of equal
    fate and crossing count, the share of the others, the relative difference of the step totals)."""
    r64, r32 = reference(case, np.float64), reference(case, np.float32)
    same = (r32["fate"] == r64["fate"]) & (r32["n_hits"] == r64["n_hits"])
    return KC.distance(r32, r64, same), float((~same).mean())


@functools.lru_cache(maxsize=None)
def schwarzschild_reference(case):
    """The binary64 frame of the Schwarzschild march of a SCHWARZSCHILD case: observer_ref's or projection_ref's."""
    import observer_ref as R
    import projection_ref as P
    sky, tex = KC.scene()
    kw = dict(h_base=KC.STEP, r_inner=KC.R_INNER, r_outer=KC.R_OUTER, sky_shift_on=case.sky)
    if case.projection:
        out = P.render(camera(case), case.projection, case.pfov, beta_of(case), sky, tex, **kw)
    else:
        out = R.render(camera(case), beta_of(case), sky, tex, **kw)
    out = {k: out[k] for k in ("bg", "disk", "fate", "n_hits")}
    out["final"] = np.clip(out["bg"] + out["disk"], 0.0, 1.0)
    for v in out.values():
        v.setflags(write=False)
    return out


def schwarzschild_distance(case):
    """(per-layer binary64 distance between kerr_observer_ref at A = 0 and the Schwarzschild reference of the same view and velocity,
    over the pixels of equal fate and crossing count; the share of the others)."""
    kerr, schw = reference(case), schwarzschild_reference(case)
    same = (kerr["fate"] == schw["fate"]) & (kerr["n_hits"] == schw["n_hits"])
    return KC.distance(kerr, schw, same), float((~same).mean())
