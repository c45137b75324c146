"""The frames the Kerr tests share: spins and views of the device test, and their kerr_ref frames, each computed once."""
import functools
import typing

import numpy as np

import kerr_ref as K

W, H, FOV, STEP = 96, 64, 90.0, 0.1
R_INNER, R_OUTER, R_MAX = 2.0, 15.0, 10.0
SPINS = (0.0, 0.6, -0.9, 0.998)
VIEWS = ((6.0, 0.0, 0.5), (3.0, 2.0, 0.3))
CASES = tuple((A, v) for A in SPINS for v in VIEWS)


@functools.lru_cache(maxsize=None)
def scene():
    from bhr_amd import scenes
    return scenes.analytic_skybox(), scenes.noisy_disk()


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64, width=W, height=H):
    """kerr_ref's frame of a case (read-only: shared between tests)."""
    A, view = case
    sky, tex = scene()
    cam = K.build_camera(list(view), FOV, width, height, R_MAX)
    out = K.render(cam, A, sky, tex, h_base=STEP, r_inner=R_INNER, r_outer=R_OUTER, dtype=dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------- the edge cases
class Edge(typing.NamedTuple):
    """A case of tests/test_gpu_kerr_edges.py: what CASES fixes -- fov, inner radius, the disk's roll, frame size, redshift,
    disk texture -- is a field here.  The roll is given the way the video loop gives it, as a frame number and the disk's
    rotation speed; t_offset is the float32 product the camera block carries."""
    A: float
    view: tuple
    fov: float = FOV
    r_inner: float = R_INNER
    frame: int = 0
    speed: float = 0.1
    width: int = W
    height: int = H
    redshift: str = "model"
    force: bool = False          # the Kerr kernel at A = 0
    disk: str = "noisy"          # "rings": a texture that is constant along phi

    @property
    def t_offset(self):
        return float(np.float32(float(self.frame) * self.speed))

    @property
    def id(self):
        s = f"A{self.A:g}-pov{self.view[0]:g}_{self.view[1]:g}_{self.view[2]:g}"
        for name, fmt in (("fov", "fov{:g}"), ("r_inner", "ri{:g}"), ("frame", "f{}"), ("speed", "v{:g}"), ("width", "w{}"),
                          ("height", "h{}"), ("redshift", "{}"), ("disk", "{}")):
            if getattr(self, name) != Edge._field_defaults[name]:
                s += "-" + fmt.format(getattr(self, name))
        return s


@functools.lru_cache(maxsize=None)
def ring_disk(n_r=32, n_phi=64, seed=5):
    """A disk texture that does not depend on phi: colour and opacity vary from ring to ring only, so the roll cannot show."""
    rows = np.random.default_rng(seed).uniform(0.05, 1.0, size=(n_r, 1, 4)).astype(np.float32)
    rows[..., 3] = 0.05 + 0.45 * rows[..., 3]
    tex = np.ascontiguousarray(np.broadcast_to(rows, (n_r, n_phi, 4)))
    tex.setflags(write=False)
    return tex


def edge_scene(case):
    sky, tex = scene()
    return sky, (ring_disk() if case.disk == "rings" else tex)


@functools.lru_cache(maxsize=None)
def edge_reference(case, dtype=np.float64):
    """The reference frame of an Edge under its redshift (read-only: shared between tests)."""
    import kerr_redshift_ref as R
    sky, tex = edge_scene(case)
    cam = K.build_camera(list(case.view), case.fov, case.width, case.height, R_MAX)
    render = R.render if case.redshift == "exact" else K.render
    out = render(cam, case.A, sky, tex, h_base=STEP, r_inner=case.r_inner, r_outer=R_OUTER, t_offset=case.t_offset, dtype=dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


def float32_distance(case):
    """(what the float32 reference keeps from the float64 one per layer, over the pixels of equal fate and crossing count; the
    share of the others): the bar of a case is twice the first, and the second says whether the case sits on a discontinuity."""
    r64, r32 = edge_reference(case, np.float64), edge_reference(case, np.float32)
    same = (r32["fate"] == r64["fate"]) & (r32["n_hits"] == r64["n_hits"])
    return distance(r32, r64, same), float((~same).mean())


def _roll(A, view, frame, speed):
    return [Edge(A, view, frame=frame, speed=speed, redshift=m) for m in ("model", "exact")]


ROLL = _roll(0.6, VIEWS[0], 73, 0.1) + _roll(-0.9, VIEWS[1], 400, -0.1) + _roll(0.998, VIEWS[0], 3000, 0.1)
RINGS = (Edge(0.6, VIEWS[0], disk="rings"), Edge(0.6, VIEWS[0], frame=73, disk="rings"))
POLAR = Edge(0.9, (0.0, 0.0, 6.0))
EQUATORIAL = Edge(0.9, (6.0, 0.0, 0.0))
CLOSE_IN = Edge(0.998, (1.3, 0.2, 0.1), fov=120.0, r_inner=0.7)
VIEW_EDGES = [POLAR, Edge(0.9, (0.3, 0.2, 6.0)), EQUATORIAL, Edge(-0.6, (4.0, -3.0, -0.4)), CLOSE_IN,
              Edge(0.6, (40.0, 0.0, 3.0), fov=30.0), Edge(-0.9, (5.0, 1.0, 1.0), fov=150.0, width=67, height=29),
              EQUATORIAL._replace(redshift="exact"), CLOSE_IN._replace(redshift="exact")]
RAGGED_SIZES = ((61, 43), (33, 9), (8, 8), (5, 3))
RAGGED = [Edge(0.9, VIEWS[1], width=w, height=h) for w, h in RAGGED_SIZES] + [Edge(0.9, VIEWS[1], width=61, height=43, redshift="exact")]
CROSSINGS = [Edge(0.998, VIEWS[0], fov=40.0, r_inner=0.7), Edge(0.0, VIEWS[0], fov=40.0, r_inner=1.0, force=True)]
MIRRORS = ((0.9, (3.0, 2.0, 0.3)), (0.6, (0.0, 0.0, 6.0)), (0.998, (4.0, -3.0, -0.4)))     # (A, (x, y, z)) against (-A, (x, -y, z))
UP_DOWN = [Edge(A, (6.0, 0.0, 0.0), redshift=m) for A in (0.9, -0.6) for m in ("model", "exact")]
INSIDE_STATIC_LIMIT = ((0.998, (1.08, 0.0, 0.05)), (0.998, (0.7, 0.0, 0.02)))            # the second is inside the horizon too


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))


def distance(got, ref, same):
    """Per-layer RMSE over the pixels `same` (those whose fate and crossing count agree)."""
    return {k: rmse(got[k][same], ref[k][same]) for k in ("bg", "disk", "final")}
