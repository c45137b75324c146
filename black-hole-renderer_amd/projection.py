"""The projections of ``--projection`` / ``HipRenderer.render_async(projection=...)``: the argument check and the frame-size rule.
No device is needed for any of this.

``equirect`` is the equirectangular panorama (360 x 180 degrees: the full sphere, what VR players open), ``fisheye`` the
equidistant fisheye whose image circle is inscribed in the frame's shorter side (180 degrees: a dome master).  include/bhr.h
(bhr_render_projected) states the model.
"""
import math

KINDS = ("equirect", "fisheye")
CHOICES = ("perspective",) + KINDS                 # the command line's names; perspective is the pinhole camera, no projection
DEFAULT_FOV = {"equirect": (360.0, 180.0), "fisheye": (180.0,)}
FOV_MAX = {"equirect": (360.0, 180.0), "fisheye": (360.0,)}


def check(projection, projection_fov=None) -> tuple:
    """(kind, fov_h, fov_v) of a projection; ValueError for an unknown kind, the wrong number of angles, a NaN or an angle outside
    (0, 360] (equirect's vertical one: (0, 180]).  ``projection_fov``: (h, v) for equirect, (full_angle,) for fisheye -- a bare
    number is taken as one angle -- None: the defaults, (360, 180) and (180,).  The fisheye's fov_v is reported as 0."""
    if projection not in KINDS:
        raise ValueError(f"projection must be one of {KINDS}, got {projection!r}")
    if projection_fov is None:
        fov = DEFAULT_FOV[projection]
    else:
        try:
            fov = tuple(float(v) for v in projection_fov) if not isinstance(projection_fov, (int, float)) else (float(projection_fov),)
        except TypeError:
            raise ValueError(f"projection_fov must be numbers, got {projection_fov!r}")
    want = len(FOV_MAX[projection])
    if len(fov) != want:
        raise ValueError(f"projection {projection} takes projection_fov = " + ("(h, v)" if want == 2 else "(full_angle,)") + f", got {projection_fov!r}")
    for v, top in zip(fov, FOV_MAX[projection]):
        if not (0.0 < v <= top) or math.isnan(v):
            raise ValueError(f"projection {projection}: projection_fov {list(fov)}: {v:g} is outside (0, {top:g}] degrees")
    return projection, fov[0], (fov[1] if want == 2 else 0.0)


def full_sphere(projection, projection_fov=None) -> bool:
    """Whether the frame covers the whole sphere as a 360-degree player expects it: equirect at 360 x 180."""
    if projection != "equirect":
        return False
    _, h, v = check(projection, projection_fov)
    return h == 360.0 and v == 180.0


def frame_size(projection, width: int, height: int) -> tuple:
    """The frame of a projection from a resolution's width x height: equirect width x width / 2 (fhd: 1920 x 960), fisheye
    height x height (fhd: 1080 x 1080); None or "perspective": the resolution itself."""
    if projection in (None, "perspective"):
        return int(width), int(height)
    if projection == "equirect":
        return int(width), int(width) // 2
    if projection == "fisheye":
        return int(height), int(height)
    raise ValueError(f"projection must be one of {KINDS}, got {projection!r}")
