"""The moving observer of ``--observer`` / ``HipRenderer.render_async(observer=...)``: named velocities, the infall path and the
validity checks.  No device is needed for any of this.

Units r_s = 1, M = 1/2.  A velocity is beta, a 3-vector in units of c as the static observer at the camera position measures it,
in that observer's local frame identified with the coordinate axes (include/bhr.h: bhr_render_observer states the model).
"""
import math

import numpy as np

BETA_MAX = 0.995
KINDS = ("static", "circular", "infall")
SKY = ("shift", "plain")
CIRCULAR_R_MIN = 1.5 + 1e-3          # no circular geodesic at or inside the photon sphere (and beta -> 1 towards it)
INFALL_R_MIN = 1.05                  # the infall path ends outside the horizon (beta = sqrt(1 / r) <= 0.976 there)


def check_beta(beta) -> tuple:
    """beta as three floats; ValueError for anything but three numbers, a NaN or |beta| > 0.995."""
    try:
        b = tuple(float(v) for v in beta)
    except TypeError:
        raise ValueError(f"observer velocity must be three numbers, got {beta!r}")
    if len(b) != 3:
        raise ValueError(f"observer velocity must be three numbers, got {beta!r}")
    n = math.sqrt(sum(v * v for v in b))
    if not n <= BETA_MAX:                # NaN included
        raise ValueError(f"observer velocity {list(b)}: |beta| = {n:g}, at most {BETA_MAX} (units of c) and no NaN")
    return b


def check_sky(sky) -> str:
    if sky not in SKY:
        raise ValueError(f"observer_sky must be 'shift' or 'plain', got {sky!r}")
    return sky


def velocity(kind: str, pos) -> np.ndarray:
    """beta of a named observer at camera position ``pos`` (binary64; r = |pos|, r_hat = pos / r):
    static    0
    circular  the circular geodesic through pos that turns in the disk's sense: sqrt(0.5 / (r - 1)) normalize(r_hat x z_hat), the
              disk's v_hat = r_hat x n for the untilted normal; 0.5 at r = 3.  Refused for r <= 1.5 + 1e-3 and on the z axis
    infall    radial free fall from rest at infinity: -sqrt(1 / r) r_hat
    """
    if kind not in KINDS:
        raise ValueError(f"observer must be one of {KINDS}, got {kind!r}")
    p = np.array([float(v) for v in pos], dtype=np.float64)
    r = float(np.linalg.norm(p))
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError(f"observer {kind}: no camera position at {list(pos)}")
    if kind == "static":
        return np.zeros(3)
    r_hat = p / r
    if kind == "circular":
        if r <= CIRCULAR_R_MIN:
            raise ValueError(f"observer circular: no circular orbit at r = {r:g} (inside 1.5 r_s, the photon sphere; r > {CIRCULAR_R_MIN:g} is needed)")
        t = np.cross(r_hat, np.array([0.0, 0.0, 1.0]))
        n = float(np.linalg.norm(t))
        if n < 1e-9:
            raise ValueError(f"observer circular: the camera at {list(pos)} is on the z axis, the orbit's direction r_hat x z_hat vanishes there")
        b = math.sqrt(0.5 / (r - 1.0)) * t / n
    else:
        b = -math.sqrt(1.0 / r) * r_hat
    check_beta(b)
    return b


KERR_KINDS = ("static", "circular", "zamo")


def kerr_velocity(kind: str, pos, A: float) -> np.ndarray:
    """beta of a named observer at camera position ``pos`` (Kerr-Schild coordinates) around a hole of spin A = a / M, as the static
    observer there measures it (binary64; a = A / 2, M = 1/2).  From pos: w = |pos|^2 - a^2, S = sqrt(w^2 + 4 a^2 z^2),
    r^2 = (w + S) / 2, Sigma = S, sin^2 theta = (x^2 + y^2) / (r^2 + a^2), and the metric's
    g_tt = -(1 - r / Sigma), g_tphi = -a r sin^2 theta / Sigma, g_phiphi = (r^2 + a^2 + a^2 r sin^2 theta / Sigma) sin^2 theta.
    A camera with angular velocity Omega (positive in the disk's sense, the hole's for A > 0) has
    u^t = 1 / sqrt(-(g_tt + 2 g_tphi Omega + g_phiphi Omega^2)), gamma = u^t (-g_tt - g_tphi Omega) / sqrt(-g_tt),
    beta = sign(Omega) sqrt(1 - 1 / gamma^2) along (y, -x, 0) / sqrt(x^2 + y^2), the disk's v_hat = r_hat x z_hat.
    static    0
    circular  Omega = sqrt(M) / (r^1.5 + a sqrt(M)), the equatorial circular geodesic in the disk's sense; the equatorial camera
              only (|z| <= 1e-6 |pos|), refused where there is no such orbit or beta > 0.995; at A = 0 it is velocity("circular")
    zamo      Omega = -g_tphi / g_phiphi, the zero-angular-momentum (frame-dragged) observer; anywhere outside the static limit,
              0 on the axis
    infall is not offered under a spin: its direction is not radial there."""
    if kind == "infall":
        raise ValueError("observer infall under a spin: the free fall from rest at infinity is not radial around a spinning hole; "
                         f"one of {KERR_KINDS}")
    if kind not in KERR_KINDS:
        raise ValueError(f"observer under a spin must be one of {KERR_KINDS}, got {kind!r}")
    A = float(A)
    if not abs(A) <= 0.998:              # NaN included
        raise ValueError(f"spin a / M = {A!r} (|a / M| <= 0.998)")
    p = np.array([float(v) for v in pos], dtype=np.float64)
    n = float(np.linalg.norm(p))
    if not (n > 0.0 and math.isfinite(n)):
        raise ValueError(f"observer {kind}: no camera position at {list(pos)}")
    if kind == "static":
        return np.zeros(3)
    M, a = 0.5, 0.5 * A
    x, y, z = p
    w = n * n - a * a
    S = math.sqrt(w * w + 4.0 * a * a * z * z)
    r2 = 0.5 * (w + S)
    r = math.sqrt(r2)
    s2 = (x * x + y * y) / (r2 + a * a)
    g_tt = -(1.0 - r / S)
    g_tp = -a * r * s2 / S
    g_pp = (r2 + a * a + a * a * r * s2 / S) * s2
    if not g_tt < 0.0:
        raise ValueError(f"observer {kind}: the camera at {list(pos)} lies inside the static limit of the hole of spin {A:g}")
    if kind == "circular":
        if abs(z) > 1e-6 * n:
            raise ValueError(f"observer circular under a spin: the camera at {list(pos)} is off the equatorial plane, where no circular geodesic lies")
        om = math.sqrt(M) / (r ** 1.5 + a * math.sqrt(M))
    else:
        if not g_pp > 0.0:               # on the axis: the frame-dragged observer is the static one
            return np.zeros(3)
        om = -g_tp / g_pp
    rad = -(g_tt + 2.0 * g_tp * om + g_pp * om * om)
    if not rad > 0.0:
        raise ValueError(f"observer {kind}: no such orbit at r = {r:g} around the hole of spin {A:g} (inside its photon orbit)")
    # sign(Omega) sqrt(1 - 1 / gamma^2) without its cancellation at small beta: 1 - 1 / gamma^2 is
    # Omega^2 (g_tphi^2 - g_tt g_phiphi) / (g_tt + g_tphi Omega)^2 identically, which is 0 where Omega is
    beta = om * math.sqrt(g_tp * g_tp - g_tt * g_pp) / (-g_tt - g_tp * om)
    if abs(beta) > BETA_MAX:
        raise ValueError(f"observer {kind}: beta = {beta:g} at r = {r:g} around the hole of spin {A:g}, at most {BETA_MAX}")
    rho = math.sqrt(x * x + y * y)
    return beta * np.array([y / rho, -x / rho, 0.0])


def kerr_frame_plan(n_frames: int, pov, A: float, kind=None, beta=None, orbit: bool = False, orbit_degrees: float = 360.0) -> list:
    """frame_plan for the spinning hole: [(camera position, beta)] with kerr_velocity(kind, position, A) at every frame's own
    position, or the fixed ``beta``."""
    from .camera import orbit_position
    positions = [[float(v) for v in (orbit_position(pov, f, n_frames, orbit_degrees) if orbit else pov)] for f in range(n_frames)]
    if beta is not None:
        b = check_beta(beta)
        return [(pos, b) for pos in positions]
    return [(pos, tuple(float(v) for v in kerr_velocity(kind or "static", pos, A))) for pos in positions]


def infall_radii(r0: float, r1: float, n: int) -> np.ndarray:
    """Radii of an n-frame radial fall from r0 to r1, uniform in the proper time of the observer who falls from rest at
    infinity (d tau = -sqrt(r) dr): r_k = (r0^1.5 + k / (n - 1) (r1^1.5 - r0^1.5))^(2/3); one frame stays at r0."""
    r0, r1, n = float(r0), float(r1), int(n)
    if n < 1:
        raise ValueError(f"infall_radii: {n} frames")
    if not (r0 > 0.0 and r1 > 0.0 and math.isfinite(r0) and math.isfinite(r1)):
        raise ValueError(f"infall_radii: radii {r0:g}, {r1:g} must be positive and finite")
    s = np.arange(n, dtype=np.float64) / max(n - 1, 1)
    r = (r0 ** 1.5 + s * (r1 ** 1.5 - r0 ** 1.5)) ** (2.0 / 3.0)
    r[0] = r0
    if n > 1:
        r[-1] = r1
    return r


def check_infall_to(pov, infall_to: float) -> float:
    R, r0 = float(infall_to), float(np.linalg.norm(np.array(pov, dtype=np.float64)))
    if not R >= INFALL_R_MIN:
        raise ValueError(f"infall_to {infall_to!r}: the fall ends outside the horizon, at R >= {INFALL_R_MIN}")
    if not R <= r0:
        raise ValueError(f"infall_to {R:g} lies outside the camera's radius {r0:g}: the camera falls inwards")
    return R


def frame_plan(n_frames: int, pov, kind=None, beta=None, orbit: bool = False, orbit_degrees: float = 360.0, infall_to=None) -> list:
    """[(camera position, beta)] of the frames of a video: the positions render_video walks -- pov, its orbit, or with
    ``infall_to`` the radial path from |pov| to it along pov -- and at each the named velocity ``kind`` evaluated there, or the
    fixed ``beta``."""
    from .camera import orbit_position
    if infall_to is not None and orbit:
        raise ValueError("infall_to moves the camera radially: it does not combine with orbit")
    if infall_to is not None:
        p = np.array([float(v) for v in pov], dtype=np.float64)
        r0 = float(np.linalg.norm(p))
        positions = [[float(v) for v in p * (r / r0)] for r in infall_radii(r0, check_infall_to(pov, infall_to), n_frames)]
    else:
        positions = [[float(v) for v in (orbit_position(pov, f, n_frames, orbit_degrees) if orbit else pov)] for f in range(n_frames)]
    if beta is not None:
        b = check_beta(beta)
        return [(pos, b) for pos in positions]
    return [(pos, tuple(float(v) for v in velocity(kind or "static", pos))) for pos in positions]
