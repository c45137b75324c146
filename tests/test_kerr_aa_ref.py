"""The CPU reference of the Kerr anti-aliasing (tests/kerr_aa_ref.py) against what can be known without it: central differences
of kerr_ref.rhs and initial_momentum, central differences of marched rays, the integrator's order, the oracle's strict
anti-aliased frame at spin 0 -- and the inputs of the device test (tests/test_gpu_kerr_aa.py): every mip level is used, and
few pixels sit near a jump of the level.

Bars are the measurement with the margin tests/test_kerr_ref.py gives its gradient check (measured 1.0e-9, bar 1e-7: a
hundredfold); each test prints what it measures."""
import numpy as np
import pytest

import kerr_aa_cases as AC
import kerr_aa_ref as AA
import kerr_cases as KC
import kerr_ref as K

SPINS = (0.0, 0.5, -0.9, 0.998)
POV, GRID = [6.0, 0.0, 0.5], 8
PROBE_ALPHA = float(1.0 - 0.5 ** (1.0 / 6.0))        # disk_alpha = 1 - (1 - alpha)^6 = 1/2

def _random_states(A, n, seed):
    rng = np.random.default_rng(seed)
    r = rng.uniform(1.2, 20.0, n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    x = u * r[:, None]
    return x, K.initial_momentum(x, d, A * K.M), d, rng


def _rel(num, ana):
    return float((np.abs(num - ana).max(1) / np.abs(ana).max(1)).max())


@pytest.mark.parametrize("A", SPINS)
def test_tangent_rhs_equals_central_differences(A):
    """Measured 7.0e-10 (dx) and 8.6e-10 (dp) at most over the four spins; bar 1e-7."""
    a = A * K.M
    x, p, _, rng = _random_states(A, 200, 7)
    xi, pi = rng.normal(size=(200, 3)), rng.normal(size=(200, 3))
    tv, tdp = AA.rhs_tangent(x, p, xi, pi, a)
    eps = 1e-5
    vp, dpp = K.rhs(x + eps * xi, p + eps * pi, a)
    vm, dpm = K.rhs(x - eps * xi, p - eps * pi, a)
    rel_v, rel_p = _rel((vp - vm) / (2 * eps), tv), _rel((dpp - dpm) / (2 * eps), tdp)
    print(f"A={A}: tangent right-hand side against central differences: dx {rel_v:.3g}, dp {rel_p:.3g}")
    assert rel_v < 1e-7 and rel_p < 1e-7


@pytest.mark.parametrize("A", SPINS)
def test_seeds_equal_central_differences(A):
    """Measured 3.6e-10 at most over the four spins; bar 5e-8."""
    a = A * K.M
    x, _, d, rng = _random_states(A, 200, 7)
    dd = 0.01 * rng.normal(size=(200, 3))
    eps = 1e-3
    num = (K.initial_momentum(x, d + eps * dd, a) - K.initial_momentum(x, d - eps * dd, a)) / (2 * eps)
    rel = _rel(num, AA.seed_tangent(x, d, dd, a))
    print(f"A={A}: seeds against central differences of initial_momentum: {rel:.3g}")
    assert rel < 5e-8


def _grid_camera():
    return K.build_camera(POV, 90.0, GRID, GRID, 10.0)


@pytest.mark.parametrize("A", SPINS)
def test_marched_tangents_equal_central_differences_of_marched_rays(A):
    """Along the 8 x 8 grid of pov (6, 0, 0.5), per pixel axis: the rays offset by +-eps pixel, marched with the base ray's recorded
    step sequence (h is a constant of the step), against the base ray's tangent seeded with the same direction derivative -- at
    every step in which all three are alive, relative to the tangent (floor 1e-3).  The difference is the central difference's
    own eps^2 term: measured 1.9e-9, 5.2e-7, 4.9e-6, 4.8e-6 for the four spins at eps = 1e-5 (a hundred times that at 1e-4);
    bar 5e-4."""
    cam, eps, n = _grid_camera(), 1e-5, GRID * GRID
    x0 = cam["pos"].astype(np.float64)
    d0 = AA.pixel_rays_diff(cam)[0].reshape(-1, 3)
    worst = 0.0
    for off in ((eps, 0.0), (0.0, eps)):
        dp = AA.pixel_rays_diff(cam, offset=off)[0].reshape(-1, 3)
        dm = AA.pixel_rays_diff(cam, offset=(-off[0], -off[1]))[0].reshape(-1, 3)
        dd = (dp - dm) / (2 * eps)
        base = AA.march(x0, d0, np.stack([dd, dd]), A, 0.1, cam["r_escape"], record=True)
        hs = []
        for idx, h, _, _ in base["path"]:
            full = np.zeros(n)
            full[idx] = h
            hs.append(full)
        plus = AA.march(x0, dp, np.stack([dd, dd]), A, 0.1, cam["r_escape"], record=True, h_given=hs)["path"]
        minus = AA.march(x0, dm, np.stack([dd, dd]), A, 0.1, cam["r_escape"], record=True, h_given=hs)["path"]
        compared = 0
        for k, (idx, _, _, nxi) in enumerate(base["path"][:min(len(plus), len(minus))]):
            (ip, _, xp, _), (im, _, xm, _) = plus[k], minus[k]
            common = np.intersect1d(np.intersect1d(idx, ip), im)
            if common.size == 0:
                continue
            num = (xp[np.searchsorted(ip, common)] - xm[np.searchsorted(im, common)]) / (2 * eps)
            ana = nxi[0][np.searchsorted(idx, common)]
            worst = max(worst, float((np.abs(num - ana).max(1) / np.maximum(np.abs(ana).max(1), 1e-3)).max()))
            compared += common.size
        assert compared > 50 * n                   # every ray, over most of its steps
    print(f"A={A}: marched tangents against central differences of marched rays: {worst:.3g}")
    assert worst < 5e-4


def _tangents_at(A, h, length=8.0):
    cam = _grid_camera()
    d, ddx, ddy = AA.pixel_rays_diff(cam)
    n_steps = int(round(length / h))
    m = AA.march(cam["pos"].astype(np.float64), d.reshape(-1, 3), np.stack([ddx.reshape(-1, 3), ddy.reshape(-1, 3)]), A, 0.1,
                 cam["r_escape"], record=True, h_given=[np.full(GRID * GRID, h)] * n_steps)
    assert len(m["path"]) == n_steps
    idx, _, _, nxi = m["path"][-1]
    out = np.full((GRID * GRID, 6), np.nan)
    out[idx] = nxi.transpose(1, 0, 2).reshape(-1, 6)
    return out


def _first_hit_differentials(A, step):
    cam = _grid_camera()
    d, ddx, ddy = AA.pixel_rays_diff(cam)
    m = AA.march(cam["pos"].astype(np.float64), d.reshape(-1, 3), np.stack([ddx.reshape(-1, 3), ddy.reshape(-1, 3)]), A, step, cam["r_escape"])
    rows = m["hits"][m["hits"][:, 1] == 0]
    out = np.full((GRID * GRID, 4), np.nan)
    out[rows[:, 0].astype(np.int64)] = rows[:, 7:11]
    return out


@pytest.mark.parametrize("A", SPINS)
def test_convergence_under_step_halving(A):
    """The tangents at a fixed affine parameter (8 r_s from the camera, constant steps 0.1, 0.05, 0.025) converge at the
    integrator's order: halving the step shrinks what they move by 2^4 (measured 14.2 .. 15.7 per ray over the four spins; the
    bar is 8, half an order less).  A HIT differential is by convention the tangent at the end of the crossing step, which lies up
    to one step behind the plane: it moves at FIRST order in the step (measured: the median ratio is 2.015 at every spin), and
    that order is asserted too -- it is what makes a lod depend on where the steps fall."""
    t1, t2, t4 = (_tangents_at(A, h) for h in (0.1, 0.05, 0.025))
    ok = np.isfinite(t1).all(1) & np.isfinite(t2).all(1) & np.isfinite(t4).all(1)
    e12, e24 = np.abs(t1 - t2)[ok].max(1), np.abs(t2 - t4)[ok].max(1)
    print(f"A={A}: {int(ok.sum())} rays; tangents move by {e12.max():.3g} then {e24.max():.3g}: ratios {(e12 / e24).min():.2f} .. {(e12 / e24).max():.2f}")
    assert ok.sum() >= 40 and (e12 / e24).min() > 8.0
    h1, h2, h4 = (_first_hit_differentials(A, s) for s in (0.1, 0.05, 0.025))
    ok = np.isfinite(h1).all(1) & np.isfinite(h2).all(1) & np.isfinite(h4).all(1)
    ratio = float(np.median(np.abs(h1 - h2)[ok].max(1) / np.abs(h2 - h4)[ok].max(1)))
    print(f"A={A}: {int(ok.sum())} first crossings; hit differentials: median ratio {ratio:.3f}")
    assert ok.sum() >= 40 and 1.8 < ratio < 2.25


def _oracle_layers(oracle, sky, tex, view):
    o = oracle.OracleRenderer(KC.W, KC.H, sky, tex, step_size=KC.STEP, r_max=KC.R_MAX, r_disk_inner=KC.R_INNER, r_disk_outer=KC.R_OUTER,
                              disk_tilt=0.0, anti_alias="lod_radius", aa_strength=1.0)
    _, img, disk, _ = o.render(list(view), KC.FOV, skip_differentials=False, skip_bloom=True, parts=True)
    out = dict(bg=img.transpose(1, 0, 2), disk=disk.transpose(1, 0, 2))
    out["final"] = np.clip(out["bg"] + out["disk"], 0, 1)
    return out


@pytest.mark.parametrize("view", KC.VIEWS, ids=lambda v: f"pov{v[0]:g}_{v[1]:g}")
def test_spin_zero_against_the_oracle(view, oracle):
    """kerr_aa_ref at A = 0 in binary64 against the oracle's strict anti-aliased frame (kerr_aa_cases.ORACLE_DISTANCE says what differs).  The
    oracle's fates and crossing counts come from a probe frame: a white sky and a disk of opacity 1/2 per crossing."""
    sky, tex = KC.scene()
    ora = _oracle_layers(oracle, sky, tex, view)
    psky, ptex = np.ones((16, 32, 3), dtype=np.float32), np.ones((8, 16, 4), dtype=np.float32)
    ptex[..., 3] = PROBE_ALPHA
    probe = _oracle_layers(oracle, psky, ptex, view)
    bg = probe["bg"][..., 0].astype(np.float64)
    o_sky = bg > 0
    o_n = np.where(o_sky, np.rint(-np.log2(np.where(o_sky, bg, 1.0))), -1).astype(np.int64)
    r64 = AC.reference((0.0, view), np.float64)
    r_sky = r64["fate"] == 1
    same = o_sky == r_sky
    same &= np.where(o_sky & r_sky, o_n == r64["n_hits"], True)
    same &= np.where(~o_sky & ~r_sky, (probe["disk"].max(axis=2) > 0) == (r64["n_hits"] > 0), True)
    got = KC.distance(r64, ora, same & AC.away_from_jumps(r64))
    print(f"{view}: kerr_aa_ref (A = 0, f64) vs the oracle's strict anti-aliased frame: fate / count differs on {float((~same).mean()):.3%}; distance {got}")
    assert float((~same).mean()) <= 0.005
    for layer, want in AC.ORACLE_DISTANCE[view].items():
        assert got[layer] == pytest.approx(want, rel=0.02), layer       # the recorded figure, to its digits


def test_device_test_inputs():
    """On the two views of kerr_cases.CASES with noisy_disk: every level 0..3 is chosen on at least 1 % of the shaded crossings
    (measured: level 1 is the rarest, 1.5 % .. 3.5 %); DELTA is four times the largest |lod32 - lod64| of the reference, at
    least 1e-3 (measured 8.2e-5: the floor holds); and the pixels with a crossing within DELTA of a jump are at most 5 % of the
    pixels that have a crossing (measured 0.05 % at most)."""
    worst = 0.0
    for case in KC.CASES:
        r64, r32 = AC.reference(case, np.float64), AC.reference(case, np.float32)
        level = AA.level_of(r64["lods"][:, 2], 3)
        shares = [float((level == k).mean()) for k in range(4)]
        worst = max(worst, AC.lod_difference(r32, r64))
        near = ~AC.away_from_jumps(r64)
        share = near.sum() / (r64["n_hits"] > 0).sum()
        print(f"{case}: level shares {[f'{s:.3f}' for s in shares]}; near a jump {share:.4%} of the pixels with a crossing")
        assert min(shares) >= 0.01
        assert share <= AC.JUMP_SHARE
    print(f"largest |lod32 - lod64| {worst:.3g}; DELTA {AC.DELTA:g}")
    assert max(4.0 * worst, 1e-3) <= AC.DELTA <= 1.05 * max(4.0 * worst, 1e-3)      # that figure, and no wider


def test_level_zero_is_the_plain_reference():
    """At strength 0 every crossing samples level 0 and the frame is kerr_ref's, bit for bit; the tangents do not touch the primal:
    at strength 1 the fates, crossing counts and steps are kerr_ref's too."""
    case = KC.CASES[3]
    plain, zero, one = KC.reference(case, np.float64), AC.reference(case, np.float64, strength=0.0), AC.reference(case, np.float64)
    for layer in ("bg", "disk", "final"):
        assert np.array_equal(plain[layer], zero[layer]), layer
    for key in ("fate", "n_hits", "steps"):
        assert np.array_equal(plain[key], one[key]), key
    assert not np.array_equal(plain["disk"], one["disk"])
