"""The frames the Kerr anti-aliasing tests share: kerr_cases' spins and views with kerr_aa_ref's frames, each computed once."""
import functools

import numpy as np

import kerr_aa_ref as AA
import kerr_cases as KC
import kerr_ref as K

# Pixels near a jump of the mip level.  The level is int(clamp(lod, 0, 3)): a crossing whose lod lies within DELTA of 1, 2 or 3
# may pick another level under another rounding of the differentials, and its pixel then differs by a texel's worth, not by
# rounding.  DELTA is four times the largest |lod32 - lod64| of kerr_aa_ref over kerr_cases.CASES (float32 against float64 run,
# crossings of equal ray, rank, fate and count; measured 8.2e-5 at A = 0.6, pov (3, 2, 0.3), so 3.3e-4), and at least 1e-3: the floor.
# tests/test_kerr_aa_ref.py checks both the figure and that such pixels are at most 5 % of the pixels that have a crossing.
DELTA = 1e-3
JUMP_SHARE = 0.05

# kerr_aa_ref (binary64, A = 0) against the oracle's strict anti-aliased frame, per view of kerr_cases.VIEWS: the per-layer RMSE
# over the pixels of equal fate and crossing count that are not near a jump, as tests/test_kerr_aa_ref.py (test_spin_zero_against_the_oracle) measured it and checks it.
# The two are not the same model: the reference's variational pair keeps L^2 of the ray constant in its Jacobian
# (render.py:2526-2539) and this one differentiates the whole right-hand side; their steps do not fall on the same points
# (tests/test_kerr_ref.py) and a hit differential is the tangent at the END of the crossing step, first order in the step.  A tenth
# of the crossings pick another level (lod differs by 0.3 .. 0.6 in the middle of its range), hence distances of a texel's worth.
# tests/test_gpu_kerr_aa.py builds its spin-0 bar on these figures.
ORACLE_DISTANCE = {KC.VIEWS[0]: dict(bg=4.88e-3, disk=1.62e-2, final=1.46e-2), KC.VIEWS[1]: dict(bg=1.03e-2, disk=2.97e-2, final=2.32e-2)}


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64, strength=1.0, redshift="model", width=KC.W, height=KC.H, fov=KC.FOV, r_inner=KC.R_INNER):
    """kerr_aa_ref's frame of a case of kerr_cases.CASES (read-only: shared between tests)."""
    A, view = case
    sky, tex = KC.scene()
    cam = K.build_camera(list(view), fov, width, height, KC.R_MAX)
    out = AA.render(cam, A, sky, tex, strength=strength, redshift=redshift, h_base=KC.STEP, r_inner=r_inner, r_outer=KC.R_OUTER, dtype=dtype)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def same_fate(a, b):
    return (a["fate"] == b["fate"]) & (a["n_hits"] == b["n_hits"])


def lod_difference(r32, r64):
    """The largest |lod32 - lod64| over the crossings (ray, rank) of the pixels of equal fate and crossing count."""
    same = same_fate(r32, r64).reshape(-1)
    key = lambda rows: rows[:, 0].astype(np.int64) * 64 + rows[:, 1].astype(np.int64)
    k32, k64 = key(r32["lods"]), key(r64["lods"])
    keep32, keep64 = same[r32["lods"][:, 0].astype(np.int64)], same[r64["lods"][:, 0].astype(np.int64)]
    o32, o64 = np.argsort(k32[keep32]), np.argsort(k64[keep64])
    assert np.array_equal(k32[keep32][o32], k64[keep64][o64])
    l32, l64 = r32["lods"][keep32][o32, 2], r64["lods"][keep64][o64, 2]
    # a lod beyond the clamp picks its level whatever its rounding
    inside = (np.minimum(l32, l64) < 3.5) & (np.maximum(l32, l64) > 0.5)
    return float(np.abs(l32 - l64)[inside].max()) if inside.any() else 0.0


def away_from_jumps(ref, delta=DELTA):
    """(H, W) bool: the pixels none of whose crossings has its lod within delta of a jump of the level."""
    return ~AA.near_jump(ref["lods"], ref["fate"].shape, delta)
