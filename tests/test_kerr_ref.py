"""The CPU reference of the spinning hole (tests/kerr_ref.py) against what can be known without it: central differences of
its own Hamiltonian, the constants of motion, the analytic shadow edges of the Kerr metric, and -- at spin 0 -- the oracle's
strict Schwarzschild march in binary64.  No GPU."""
import numpy as np
import pytest

import kerr_ref as K

SPINS = [0.0, 0.5, -0.9, 0.998]

# Reduction to the oracle at A = 0 (test_spin_zero_reduces_to_the_oracle): the largest distance measured over the 16 x 12 grid
# of the view below at step 0.02 was 2.86e-5 (escape directions) and 1.24e-5 (first hit points); times 4 for other views.
# The two marches do not take the same steps: the oracle's affine parameter makes |dx/dl| = 1 at the camera, the
# Hamiltonian's (p_t = -1) makes it s = 1 / sqrt(1 - f (1 - (l.d)^2)), 1.05 at 6 r_s, so the rays end some 5 % of their
# steps apart and leave the escape sphere at slightly different points.
ORACLE_DIR_BAR = 4 * 2.86e-5
ORACLE_HIT_BAR = 4 * 1.24e-5
# The float32 reference against the float64 one on the device test's cases (tests/kerr_cases.py): pixels whose fate or
# crossing count differs stay under the 0.5 % the device test allows.
FATE_SHARE = 0.005


def _random_states(A, n, seed):
    rng = np.random.default_rng(seed)
    r = rng.uniform(1.2, 20.0, n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    x = u * r[:, None]
    return x, K.initial_momentum(x, d, A * K.M), d


@pytest.mark.parametrize("A", SPINS)
def test_gradients_equal_central_differences(A):
    a = A * K.M
    x, p, d = _random_states(A, 200, 7)
    v, dp = K.rhs(x, p, a)
    eps = 1e-5
    num_v, num_dp = np.zeros_like(v), np.zeros_like(dp)
    for k in range(3):
        e = np.zeros(3)
        e[k] = eps
        num_dp[:, k] = -(K.hamiltonian(x + e, p, a) - K.hamiltonian(x - e, p, a)) / (2 * eps)
        num_v[:, k] = (K.hamiltonian(x, p + e, a) - K.hamiltonian(x, p - e, a)) / (2 * eps)
    rel_p = (np.abs(num_dp - dp).max(1) / np.abs(dp).max(1)).max()
    rel_x = (np.abs(num_v - v).max(1) / np.abs(v).max(1)).max()
    print(f"A={A}: gradient error dp {rel_p:.3g}, dx {rel_x:.3g}")
    assert rel_p < 1e-7 and rel_x < 1e-7
    # the camera's momentum: a null ray (H = 0) whose coordinate velocity is parallel to d
    assert np.abs(K.hamiltonian(x, p, a)).max() < 1e-12
    assert np.abs(np.cross(v, d)).max() < 1e-12


# Conservation (test_h_and_lz_are_conserved).  Captured rays plunge through r < 1.5 r_s, where the reference's step rule stops
# refining the step (dt_fac's floor) and RK4 at step 0.05 cannot hold 1e-6: measured on the 12 captured rays of the 8 x 8 grid,
# the largest |H - H0|, |L_z - L_z0| outside the horizon, per spin.  The plunging part is held to four times that, and to the
# order of the integrator: halving the step must shrink both drifts at least fourfold (RK4 gives 16, measured 5.2 .. 21; an
# error in a gradient or a sign leaves a drift that does not shrink with the step at all).
PLUNGE_DRIFT = {0.0: (1.61e-6, 2.23e-7), 0.5: (8.22e-6, 7.05e-7), -0.9: (1.55e-4, 4.23e-6), 0.998: (1.85e-3, 1.61e-5)}


def _drifts(cam, d, A, step, **kw):
    return K.march(cam["pos"].astype(np.float64), d, A, h_base=step, r_escape=cam["r_escape"], want_path=True, **kw)


@pytest.mark.parametrize("A", SPINS)
def test_h_and_lz_are_conserved(A):
    """H and L_z within 1e-6 of their initial values along 64 rays at step 0.05: the 64 rays of a 12 x 12 grid nearest to the
    hole among those the analytic shadow edge says reach the sky whatever the spin (|x cross d| > 3.7: the largest critical
    L_z / E is 3.49, the polar extent of the shadow 2.6).  Then every ray of the 8 x 8 grid of the same view: 1e-6 on those
    that reach the sky, strongly deflected ones included, and the plunging ones as stated above PLUNGE_DRIFT."""
    cam = K.build_camera([6.0, 0.0, 0.5], 90.0, 12, 12)
    d = K.pixel_rays(cam).reshape(-1, 3)
    b = np.linalg.norm(np.cross(np.broadcast_to(cam["pos"].astype(np.float64), d.shape), d), axis=1)
    far = np.nonzero(b > 3.7)[0]
    far = far[np.argsort(b[far], kind="stable")][:64]
    assert far.size == 64
    m = _drifts(cam, d[far], A, 0.05)
    print(f"A={A}: 64 rays with b in [{b[far].min():.2f}, {b[far].max():.2f}]: max |H - H0| {m['dH'].max():.3g}, max |L_z - L_z0| {m['dL'].max():.3g}")
    assert (m["fate"] == 1).all()
    assert m["dH"].max() < 1e-6 and m["dL"].max() < 1e-6

    cam = K.build_camera([6.0, 0.0, 0.5], 90.0, 8, 8)
    d = K.pixel_rays(cam).reshape(-1, 3)
    m, half = _drifts(cam, d, A, 0.05), _drifts(cam, d, A, 0.025)
    seen, lost = m["fate"] == 1, m["fate"] == 0
    assert (seen | lost).all() and np.array_equal(m["fate"], half["fate"]) and seen.sum() >= 48 and lost.sum() >= 8
    ratio_h, ratio_l = m["dH"][lost] / half["dH"][lost], m["dL"][lost] / half["dL"][lost]
    print(f"A={A}: 8 x 8 grid: {int(seen.sum())} rays reach the sky: {m['dH'][seen].max():.3g}, {m['dL'][seen].max():.3g}; {int(lost.sum())} plunge: "
          f"{m['dH'][lost].max():.3g}, {m['dL'][lost].max():.3g}, at half the step {half['dH'][lost].max():.3g}, {half['dL'][lost].max():.3g} "
          f"(ratios {ratio_h.min():.1f} .. {ratio_h.max():.1f}, {ratio_l.min():.1f} .. {ratio_l.max():.1f})")
    assert m["dH"][seen].max() < 1e-6 and m["dL"][seen].max() < 1e-6
    bar_h, bar_l = PLUNGE_DRIFT[A]
    assert m["dH"][lost].max() <= 4 * bar_h and m["dL"][lost].max() <= 4 * bar_l
    assert ratio_h.min() >= 4 and ratio_l.min() >= 4


def _equatorial(alpha):
    return np.stack([-np.cos(alpha), np.sin(alpha), np.zeros_like(alpha)], axis=-1)


def _edge(A, b_want, x0):
    """L_z / E at the capture boundary nearest to b_want on the equatorial row: two rounds of 256 rays, first across
    b_want +- 0.05, then across the pair of neighbours the boundary lies between."""
    a = A * K.M

    def lz_of(alpha):
        return K.l_z(np.broadcast_to(x0, (alpha.size, 3)), K.initial_momentum(np.broadcast_to(x0, (alpha.size, 3)), _equatorial(alpha), a))
    # the angle of a given L_z: bisection on the camera's own momentum (monotonic in alpha)
    def alpha_of(b):
        lo, hi = -1.2, 1.2
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if lz_of(np.array([mid]))[0] < b else (lo, mid)
        return 0.5 * (lo + hi)
    lo, hi = alpha_of(b_want - 0.05), alpha_of(b_want + 0.05)
    for _ in range(2):
        al = np.linspace(lo, hi, 256)
        fate = K.march(x0, _equatorial(al), A, h_base=0.05, r_escape=12.0)["fate"]
        assert set(np.unique(fate)) <= {0, 1}
        flips = np.nonzero(fate[1:] != fate[:-1])[0]
        assert flips.size == 1, f"A={A}: {flips.size} capture boundaries in the bracket"
        lo, hi = al[flips[0]], al[flips[0] + 1]
    b = lz_of(np.array([lo, hi]))
    return float(b.mean()), float(abs(b[1] - b[0]))


@pytest.mark.parametrize("A", [0.5, 0.9, -0.9])
def test_shadow_edges_are_the_analytic_ones(A):
    x0 = np.array([6.0, 0.0, 0.0])
    b_pro, b_retro = K.shadow_edges(abs(A))
    if A == 0.5:
        assert abs(b_pro - 2.0481333) < 1e-6 and abs(b_retro + 3.0690779) < 1e-6
    # positive spin: the small edge is on the d_y > 0 side (L_z > 0); negative spin mirrors it
    want = (b_pro, b_retro) if A > 0 else (-b_retro, -b_pro)
    assert K.shadow_edges(A) == pytest.approx(want, abs=1e-12)
    small = min(want, key=abs)
    assert (small > 0) == (A > 0)
    for b in want:
        got, width = _edge(A, b, x0)
        print(f"A={A}: edge {got:.7f} (bracket {width:.1e}), analytic {b:.7f}, off by {got - b:.2e}")
        assert width < 5e-6
        assert abs(got - b) < 1e-5


def _oracle_grid(oracle):
    from bhr_amd import scenes
    W, H = 16, 12
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    o = oracle.OracleRenderer(W, H, sky, tex, step_size=0.02, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, fast="f64")
    return o, W, H


def test_spin_zero_reduces_to_the_oracle(oracle):
    """At A = 0 the Hamiltonian march is the oracle's strict Schwarzschild march (acceleration form), run in binary64 on
    the same 16 x 12 rays at step 0.02: escape directions and first hit points.  Rays within 0.05 of the critical impact
    parameter wind around the photon sphere and amplify the two forms' different truncation errors: left out, at most 5 %."""
    pos, fov = [6.0, 0.0, 0.5], 90.0
    o, W, H = _oracle_grid(oracle)
    esc_o = o.escape_directions(pos, fov).transpose(1, 0, 2)                    # (H, W, 3)
    _, _, rows = o.crossings(pos, fov, skip_differentials=True)
    first_o = np.full((H, W, 2), np.nan)
    for row in rows[::-1]:                                                      # a pixel's rows are in march order: keep the first
        first_o[int(row[1]), int(row[0])] = row[2:4]
    cam = K.build_camera(pos, fov, W, H)
    ref = K.render(cam, 0.0, o.skybox, o.disk_tex, h_base=0.02)
    d = K.pixel_rays(cam)
    b = np.linalg.norm(np.cross(np.broadcast_to(cam["pos"].astype(np.float64), d.shape), d), axis=-1)
    near = np.abs(b - 1.5 * np.sqrt(3.0)) < 0.05
    assert near.mean() <= 0.05, f"{near.mean():.3f} of the grid lies near the critical impact parameter"
    use = ~near
    escaped_o = (esc_o != 0).any(-1)
    assert np.array_equal(escaped_o[use], (ref["fate"] == 1)[use])
    assert np.array_equal(np.isnan(first_o[..., 0])[use], np.isnan(ref["first_hit"][..., 0])[use])
    d_dir = np.abs(esc_o - ref["esc_dir"])[use].max()
    have = use & ~np.isnan(first_o[..., 0])
    assert escaped_o[use].sum() > 50 and have.sum() > 30
    d_hit = np.abs(first_o - ref["first_hit"])[have].max()
    print(f"A=0 against the oracle (f64, step 0.02): escape directions {d_dir:.3g}, first hits {d_hit:.3g}, left out {int(near.sum())} rays")
    assert d_dir <= ORACLE_DIR_BAR
    assert d_hit <= ORACLE_HIT_BAR


def test_float32_reference_keeps_fates_and_crossings():
    """What the device test allows for pixels whose fate or crossing count differs from the float64 run (0.5 % of a frame)
    has to cover the number format alone: the float32 reference on the same cases."""
    import kerr_cases
    for case in kerr_cases.CASES:
        r64, r32 = kerr_cases.reference(case, np.float64), kerr_cases.reference(case, np.float32)
        share = ((r64["fate"] != r32["fate"]) | (r64["n_hits"] != r32["n_hits"])).mean()
        print(f"{case}: {share:.4%} of the pixels change fate or crossing count in float32")
        assert share <= FATE_SHARE
