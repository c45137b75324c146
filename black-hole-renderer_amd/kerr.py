"""Radii of the Kerr metric in this project's units (r_s = 1, M = 1/2) and the checks of ``--spin`` / ``HipRenderer.set_spin``.

The spin is A = a / M, |A| <= 0.998; positive turns with the disk's orbital motion.  No device is needed for any of this.
"""
import math

M = 0.5
SPIN_MAX = 0.998
REDSHIFTS = ("model", "exact")


def check_redshift(mode) -> str:
    if mode not in REDSHIFTS:
        raise ValueError(f"redshift must be 'model' or 'exact', got {mode!r}")
    return mode


def check_spin(a_over_m) -> float:
    a = float(a_over_m)
    if not abs(a) <= SPIN_MAX:           # NaN included
        raise ValueError(f"spin a/M must lie in [-{SPIN_MAX}, {SPIN_MAX}], got {a_over_m!r}")
    return a


def r_plus(a_over_m: float) -> float:
    """Radius of the outer horizon, (1 + sqrt(1 - A^2)) / 2: 1 = r_s at A = 0."""
    return 0.5 * (1.0 + math.sqrt(1.0 - a_over_m * a_over_m))


def r_isco(a_over_m: float, prograde: bool) -> float:
    """Innermost stable circular orbit (Bardeen, Press, Teukolsky 1972); prograde: the orbit turns with the hole."""
    A = abs(a_over_m)
    z1 = 1.0 + (1.0 - A * A) ** (1.0 / 3.0) * ((1.0 + A) ** (1.0 / 3.0) + (1.0 - A) ** (1.0 / 3.0))
    z2 = math.sqrt(3.0 * A * A + z1 * z1)
    root = math.sqrt(max((3.0 - z1) * (3.0 + z1 + 2.0 * z2), 0.0))
    return M * (3.0 + z2 - root if prograde else 3.0 + z2 + root)


def r_photon(a_over_m: float, prograde: bool) -> float:
    """Equatorial circular photon orbit, 2 M (1 + cos(2/3 acos(-+A)))."""
    A = abs(a_over_m)
    return 2.0 * M * (1.0 + math.cos(2.0 / 3.0 * math.acos(-A if prograde else A)))


def camera_f(cam_pos, a_over_m: float) -> tuple:
    """(f, r) at a camera position: f = r / S of the Kerr-Schild form and the Kerr-Schild radius r.  f = 1 is the static limit."""
    x, y, z = (float(v) for v in cam_pos)
    a2 = (a_over_m * M) ** 2
    w = (x * x + y * y + z * z) - a2
    S = math.sqrt(w * w + 4.0 * a2 * z * z)
    r = math.sqrt(0.5 * (w + S))
    return (r / S if S > 0 else math.inf), r


def camera_outside_static_limit(cam_pos, a_over_m: float) -> bool:
    """The domain of the Kerr march's camera (include/bhr.h: bhr_set_spin): f < 1 and outside the horizon.  An orbit about the
    spin axis keeps both numbers, so a video's first camera decides for all its frames."""
    f, r = camera_f(cam_pos, a_over_m)
    return f < 1.0 and r >= r_plus(a_over_m)


def kerr_info(a_over_m: float) -> dict:
    A = check_spin(a_over_m)
    return dict(a=A * M, r_plus=r_plus(A), r_isco_prograde=r_isco(A, True), r_isco_retrograde=r_isco(A, False),
                r_photon_pro=r_photon(A, True), r_photon_retro=r_photon(A, False))


def disk_isco(a_over_m: float) -> float:
    """The ISCO of the disk's own sense of rotation: prograde for A >= 0, retrograde for a disk that turns against the hole."""
    return r_isco(a_over_m, a_over_m >= 0)


def disk_isco_orbit(a_over_m: float) -> tuple:
    """(r_isco, E, L) of the disk's sense: the radius and the energy -u_t and angular momentum u_phi of its circular orbit,
    which the gas inside it keeps under the exact redshift (the library computes the same in binary64 for its kernels)."""
    r, a, sm = disk_isco(a_over_m), a_over_m * M, math.sqrt(M)
    den = r ** 0.75 * math.sqrt(r ** 1.5 - 3.0 * M * math.sqrt(r) + 2.0 * a * sm)
    return r, (r ** 1.5 - 2.0 * M * math.sqrt(r) + a * sm) / den, sm * (r * r - 2.0 * a * sm * math.sqrt(r) + a * a) / den
