"""The frames the light-delay tests share: the cases of the device test and their delay_ref frames, each computed once."""
import functools
import typing

import numpy as np

import delay_ref as D
import kerr_ref as K
import observer_cases as OC

W, H, FOV, STEP = 96, 64, 90.0, 0.1
R_INNER, R_OUTER, R_MAX = 2.0, 15.0, 10.0
VIEWS = ((6.0, 0.0, 0.5), (3.0, 2.0, 0.3), (2.0, 1.0, 8.0))     # the two of observer_cases and one from high above the plane
TILTS = (0.0, 25.0)
ROTATION_SPEED = 0.1      # t_offset = frame * ROTATION_SPEED (HipRenderer.camera_uniforms)


class Case(typing.NamedTuple):
    name: str
    view: tuple
    scale: float
    tilt: float = 0.0
    frame: int = 0          # t_offset = frame * ROTATION_SPEED: 0 and 7.3
    texture: str = "smooth"

    @property
    def t_offset(self):
        return float(self.frame) * ROTATION_SPEED


CASES = (Case("edge_on", VIEWS[0], 1.0),
         Case("edge_on_tilt25_t7.3", VIEWS[0], 1.0, tilt=25.0, frame=73),
         Case("close_exaggerated", VIEWS[1], 2.5, frame=73),
         Case("close_tilt25", VIEWS[1], 1.0, tilt=25.0),
         Case("from_above_t7.3", VIEWS[2], 1.0, frame=73),
         Case("from_above_tilt25_exaggerated", VIEWS[2], 2.5, tilt=25.0),
         Case("noisy_texture", VIEWS[0], 1.0, frame=73, texture="noisy"))


@functools.lru_cache(maxsize=None)
def smooth_disk(n_r=64, n_phi=256):
    """A disk texture that is smooth in phi: a few azimuthal harmonics per colour channel, their phases turning slowly with the
    radius.  A phase error of the roll shows as a proportional colour error, not as flipped texels.  Alpha is between 0.3 and
    0.7 -- below 1, so the secondary image counts -- and depends on the radius alone: the sky through 1 - alpha (BG) is then the
    same under every delay, and a frame shows the delay in its DISK layer only."""
    v, phi = np.meshgrid(np.linspace(0, 1, n_r), np.linspace(0, 2 * np.pi, n_phi, endpoint=False), indexing="ij")
    red = 0.55 + 0.25 * np.sin(phi + 2.0 * v) + 0.10 * np.sin(3 * phi - 1.0)
    green = 0.50 + 0.20 * np.cos(2 * phi - 3.0 * v) + 0.10 * np.sin(5 * phi + 0.5)
    blue = 0.45 + 0.20 * np.sin(2 * phi + 1.0) + 0.15 * np.cos(4 * phi + 2.0 * v)
    alpha = 0.5 + 0.2 * np.cos(4.0 * np.pi * v)
    tex = np.ascontiguousarray(np.stack([red, green, blue, alpha], axis=-1).astype(np.float32))
    tex.setflags(write=False)
    return tex


def scene(texture="smooth"):
    """(sky, disk texture) of a case: observer_cases' sky, and its noisy disk or the smooth one."""
    sky, noisy = OC.scene()
    return sky, (noisy if texture == "noisy" else smooth_disk())


def camera(view, width=W, height=H):
    return K.build_camera(list(view), FOV, width, height, R_MAX)


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64, width=W, height=H, scale=None):
    """delay_ref's frame of a case (read-only: shared between tests); scale: instead of the case's own."""
    sky, tex = scene(case.texture)
    out = D.render(camera(case.view, width, height), case.scale if scale is None else scale, sky, tex, h_base=STEP, r_inner=R_INNER,
                   r_outer=R_OUTER, tilt_deg=case.tilt, t_offset=np.float32(case.t_offset), dtype=dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


# How far BG may move under a delay with the smooth texture.  BG is sky * (1 - alpha_total), and the delay reaches it only through
# the bilinear sample of an alpha that does not depend on phi: the four weights sum to 1 within 3 ulp of f32, so the sample moves by
# at most 3 * 2^-24 * 0.7 (alpha <= 0.7); disk_alpha = 1 - (1 - a)^6 has slope 6 (1 - a)^5 <= 6 * 0.7^5 = 1.01 for a >= 0.3; a ray
# has at most three crossings before alpha_total saturates the product, and the sky is below 1: 3 * 1.01 * 3 * 2^-24 * 0.7 < 4e-7,
# doubled for the roundings of the compositing itself.
BG_ROUNDING = 8e-7

rmse = OC.rmse
off_share = OC.off_share
