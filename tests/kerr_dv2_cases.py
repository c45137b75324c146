"""The frames the Kerr Disk V2 tests share: the cases of tests/test_gpu_kerr_disk_v2.py and their kerr_dv2_ref frames, each computed
once, and the distances tests/test_kerr_dv2_ref.py records for the device's spin-0 test."""
import functools
import typing

import numpy as np

import kerr_cases as KC
import kerr_dv2_ref as D
import kerr_ref as K

NO_STRUCTURE = dict(mode1_strength=0.0, mode2_strength=0.0, shear_strength=0.0, hotspot_strength=0.0)
SUBSTEPS = 3


class Case(typing.NamedTuple):
    """One frame: the source ("surface" or "volume"), the hole, the view, and what kerr_cases fixes where a test varies it.  The
    model is DiskV2Params(r_in=r_inner) with its defaults (r_out = 10 inside the march's r_outer = 15) unless h0 says otherwise."""
    kind: str
    A: float
    view: tuple
    redshift: str = "model"
    fov: float = KC.FOV
    r_inner: float = KC.R_INNER
    t_offset: float = 0.0
    width: int = KC.W
    height: int = KC.H
    h0: typing.Optional[float] = None
    structure: bool = True

    @property
    def id(self):
        s = f"{self.kind}-A{self.A:g}-pov{self.view[0]:g}_{self.view[1]:g}_{self.view[2]:g}"
        for name, fmt in (("redshift", "{}"), ("fov", "fov{:g}"), ("r_inner", "ri{:g}"), ("t_offset", "t{:g}"), ("width", "w{}"), ("height", "h{}"),
                          ("h0", "h0_{:g}"), ("structure", "structure{}")):
            if getattr(self, name) != Case._field_defaults[name]:
                s += "-" + fmt.format(getattr(self, name))
        return s


def params(case):
    from bhr_amd.disk_v2 import DiskV2Params, DiskV2StructureParams
    kw = {} if case.h0 is None else {"h0": case.h0}
    return DiskV2Params(r_in=case.r_inner, **kw), (None if case.structure else DiskV2StructureParams(**NO_STRUCTURE))


@functools.lru_cache(maxsize=None)
def model(r_inner=KC.R_INNER, h0=None, structure=True):
    p, sp = params(Case("surface", 0.0, KC.VIEWS[0], r_inner=r_inner, h0=h0, structure=structure))
    return D.Model(p, sp, seed=42)


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64):
    """kerr_dv2_ref's frame of a case (read-only: shared between tests)."""
    sky, _ = KC.scene()
    cam = K.build_camera(list(case.view), case.fov, case.width, case.height, KC.R_MAX)
    mdl = model(case.r_inner, case.h0, case.structure)
    kw = dict(h_base=KC.STEP, r_inner=case.r_inner, r_outer=KC.R_OUTER, t_offset=case.t_offset, dtype=dtype)
    if case.kind == "volume":
        out = D.render_volume(cam, case.A, sky, mdl, substeps=SUBSTEPS, **kw)
    else:
        out = D.render_surface(cam, case.A, sky, mdl, redshift=case.redshift, **kw)
    for v in out.values():
        v.setflags(write=False)
    return out


def float32_distance(case):
    """(what the float32 reference keeps from the float64 one per layer over the pixels of equal fate and crossing count, the
    share of the others): a case's bar is twice the first (test_gpu_kerr.py's rule)."""
    r64, r32 = reference(case, np.float64), reference(case, np.float32)
    same = (r32["fate"] == r64["fate"]) & (r32["n_hits"] == r64["n_hits"])
    return KC.distance(r32, r64, same), float((~same).mean())


# ---- the cases of the device test ---------------------------------------------------------------------------------------------
SURFACE = [Case("surface", A, v) for A, v in KC.CASES]
SURFACE_EXACT = [Case("surface", 0.6, KC.VIEWS[0], "exact"), Case("surface", -0.9, KC.VIEWS[1], "exact"), Case("surface", 0.998, KC.VIEWS[0], "exact")]
SURFACE_LATER = Case("surface", 0.6, KC.VIEWS[0], t_offset=float(np.float32(73 * 0.1)))
VOLUME = [Case("volume", 0.6, KC.VIEWS[0]), Case("volume", -0.9, KC.VIEWS[1]), Case("volume", 0.998, KC.VIEWS[0])]
VOLUME_THICK = Case("volume", 0.9, (6.0, 0.0, 2.5), h0=0.2)
CULL = [Case("volume", 0.9, (6.0, 0.0, 0.0)), Case("volume", KC.CLOSE_IN.A, KC.CLOSE_IN.view, fov=KC.CLOSE_IN.fov, r_inner=KC.CLOSE_IN.r_inner)]
RAGGED = [Case(kind, 0.9, KC.VIEWS[1], width=w, height=h) for kind in ("surface", "volume") for w, h in KC.RAGGED_SIZES]

# kerr_dv2_ref (binary64, A = 0) against the oracle's strict Schwarzschild Disk V2 frames, per-layer RMSE over the pixels of equal
# fate (tests/test_kerr_dv2_ref.py measures and pins them): the two are different integrators of the same geodesics -- RK4 on (x, p)
# against RK4 on the orbit equation, steps at other points -- so hit points, chords and escape directions differ at the steps'
# truncation order.  Twice these are the bars of the device's spin-0 test.
ORACLE_DISTANCE = {
    ("surface", KC.VIEWS[0]): dict(bg=1.88e-4, disk=2.04e-4, final=2.72e-4), ("surface", KC.VIEWS[1]): dict(bg=2.27e-3, disk=7.63e-4, final=2.20e-3),
    ("volume", KC.VIEWS[0]): dict(bg=1.91e-4, disk=1.24e-3, final=1.24e-3), ("volume", KC.VIEWS[1]): dict(bg=2.05e-3, disk=1.82e-3, final=2.67e-3),
}
