"""disk_v2 on the device against tables produced by the reference's NumPy package (tests/golden/disk_v2.npz),
plus the reference's own invariants restated (tests/unit/test_disk_v2_*.py)."""
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- CPU: parameter validation and the random tables (no device call) ---------------------------------
def test_params_validation_matches_reference():
    import bhr_amd  # noqa: F401
    from bhr_amd.disk_v2 import DiskV2Params, DiskV2StructureParams
    p = DiskV2Params()
    assert (p.r_in, p.r_out, p.h0, p.beta_h, p.rho_power, p.temp_scale, p.omega_scale, p.edge_softness) == \
        (2.0, 10.0, 0.05, 0.05, 1.0, 1.0, 1.0, 0.1)
    s = DiskV2StructureParams()
    assert (s.mode1_strength, s.mode2_strength, s.shear_strength, s.shear_components, s.hotspot_strength,
            s.hotspot_count, s.hotspot_phi_sigma, s.hotspot_logr_sigma, s.hotspot_inner_bias) == \
        (0.03, 0.05, 0.22, 8, 0.16, 8, 0.18, 0.12, 2.0)
    for kw in (dict(r_in=0.0), dict(r_out=2.0), dict(h0=0.0), dict(rho_power=0.0), dict(temp_scale=0.0),
               dict(omega_scale=-1.0), dict(edge_softness=0.5), dict(edge_softness=-0.1)):
        with pytest.raises(ValueError):
            DiskV2Params(**kw)
    for kw in (dict(mode1_strength=-0.1), dict(mode1_strength=0.6, mode2_strength=0.4), dict(shear_strength=1.0),
               dict(shear_components=0), dict(hotspot_strength=1.0), dict(hotspot_count=0),
               dict(hotspot_phi_sigma=0.0), dict(hotspot_logr_sigma=0.0), dict(hotspot_inner_bias=0.0)):
        with pytest.raises(ValueError):
            DiskV2StructureParams(**kw)


def test_random_tables_are_seed_reproducible():
    import bhr_amd  # noqa: F401
    from bhr_amd import disk_v2 as dv
    sp = dv.DiskV2StructureParams()
    assert dv.shear_table(sp, 42) == dv.shear_table(sp, 42) != dv.shear_table(sp, 43)
    t = dv.shear_table(sp, 7)
    assert len(t) == 8 and all(2 <= a < 10 and 1 <= b < 6 and 0 <= c < 2 * np.pi for a, b, c in t)
    h = dv.hotspot_table(dv.DiskV2Params(), sp, 8)
    assert len(h) == 8 and all(0.6 <= w <= 1.0 and 0 <= lr <= np.log(5.0) for _, lr, w in h)
    with pytest.raises(ValueError):
        dv.smoothstep(1.0, 1.0, 0.5)


# ---- GPU ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "disk_v2.npz"))


@pytest.fixture(scope="module")
def gold_alt():
    return np.load(os.path.join(G, "disk_v2_alt.npz"))


def _check_fields(gold, which):
    from bhr_amd import disk_v2 as dv
    import disk_v2_sets as sets
    P, _ = sets.make(which)
    r, zf = gold["r"], gold["zf"]
    H = dv.disk_half_thickness(r, P)
    tol = dict(rtol=2e-14, atol=1e-15)
    np.testing.assert_allclose(H, gold["H"], **tol)
    rr = np.repeat(r[:, None], len(zf), axis=1)
    zz = zf[None, :] * gold["H"][:, None]
    np.testing.assert_array_equal(dv.disk_radial_mask(r, P), gold["mask_r"])
    np.testing.assert_allclose(dv.disk_radial_weight(r, P), gold["W_r"], **tol)
    np.testing.assert_allclose(dv.disk_vertical_weight(rr, zz, P), gold["W_z"], **tol)
    np.testing.assert_array_equal(dv.disk_volume_mask(rr, zz, P), gold["mask_vol"])
    np.testing.assert_allclose(dv.angular_velocity_field(r, P), gold["omega"], **tol)
    np.testing.assert_allclose(dv.midplane_density_field(r, P), gold["rho_mid"], **tol)
    np.testing.assert_allclose(dv.midplane_temperature_field(r, P), gold["T_mid"], **tol)
    np.testing.assert_allclose(dv.density_field(rr, zz, P), gold["rho"], **tol)
    np.testing.assert_allclose(dv.temperature_field(rr, zz, P), gold["T"], **tol)
    np.testing.assert_allclose(dv.smoothstep(0.0, 1.0, np.linspace(-0.5, 1.5, 41)), gold["smooth"], rtol=0, atol=0)
    return P, tol


def _check_modulations(gold, which):
    from bhr_amd import disk_v2 as dv
    import disk_v2_sets as sets
    P, sp = sets.make(which)
    rg, pg = np.meshgrid(gold["rg"], gold["phig"], indexing="ij")
    tol = dict(rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(dv.weak_mode_modulation(rg, pg, P, sp), gold["F_mode"], **tol)
    for seed in (7, 42, 123):
        np.testing.assert_allclose(dv.shear_modulation(rg, pg, P, sp, seed=seed), gold[f"F_shear_{seed}"], **tol)
        np.testing.assert_allclose(dv.hotspot_modulation(rg, pg, P, sp, seed=seed), gold[f"F_hotspot_{seed}"], **tol)
        np.testing.assert_allclose(dv.structure_modulation(rg, pg, P, sp, seed=seed), gold[f"F_total_{seed}"], **tol)


@pytest.mark.gpu
def test_fields_match_reference_tables(gold, hip_lib):
    from bhr_amd import disk_v2 as dv
    P, tol = _check_fields(gold, "default")
    probe = [dv.disk_half_thickness(3.0, P), dv.disk_radial_weight(2.0, P), dv.disk_radial_weight(10.0, P),
             dv.angular_velocity_field(2.0, P), dv.midplane_temperature_field(2.0, P), dv.density_field(4.0, 0.0, P)]
    assert all(isinstance(v, float) for v in probe)                       # scalars in, scalars out
    np.testing.assert_allclose(probe, gold["scalar_probe"], **tol)


@pytest.mark.gpu
def test_modulations_match_reference_tables(gold, hip_lib):
    _check_modulations(gold, "default")


@pytest.mark.gpu
def test_fields_match_reference_tables_alt(gold_alt, hip_lib):
    """The second parameter set (tests/disk_v2_sets.py): radii 0.5 r_in .. 1.2 r_out with r_in and r_out among them."""
    _check_fields(gold_alt, "alt")


@pytest.mark.gpu
def test_modulations_match_reference_tables_alt(gold_alt, hip_lib):
    """32 shear components and 32 hotspots, angles over [-40, 40]."""
    _check_modulations(gold_alt, "alt")


@pytest.mark.gpu
def test_reference_invariants(hip_lib):
    """tests/unit/test_disk_v2_physical_fields.py / _structure_modulations.py restated."""
    from bhr_amd import disk_v2 as dv
    P = dv.DiskV2Params()
    r = np.linspace(2.0, 10.0, 257)
    om = dv.angular_velocity_field(r, P)
    assert np.all(np.diff(om) < 0)                                         # Omega decreases outwards
    assert dv.disk_radial_weight(2.0, P) == 0.0 and dv.disk_radial_weight(10.0, P) == 0.0   # exact boundaries
    assert dv.disk_radial_mask(2.0, P) and dv.disk_radial_mask(10.0, P) and not dv.disk_radial_mask(10.0001, P)
    T = dv.midplane_temperature_field(r, P)
    assert T[0] == 0.0 and r[np.argmax(T)] > P.r_in                        # peak outside r_in
    H = dv.disk_half_thickness(r, P)
    assert np.all(dv.density_field(r, 1.1 * H, P) == 0.0)                   # above the surface
    assert np.all(dv.density_field(r[1:-1], 0.0, P) > 0.0)
    rg, pg = np.meshgrid(np.linspace(1.0, 12.0, 40), np.linspace(0, 2 * np.pi, 64, endpoint=False), indexing="ij")
    F = dv.structure_modulation(rg, pg, P, seed=5)
    outside = (rg <= P.r_in) | (rg >= P.r_out)
    assert np.all(F[outside] == 1.0) and np.all(F > 0)                      # neutral outside, positive inside
    np.testing.assert_array_equal(F, dv.structure_modulation(rg, pg, P, seed=5))
    assert np.abs(F - dv.structure_modulation(rg, pg, P, seed=6)).max() > 1e-3


@pytest.mark.gpu
def test_fixed_normalisation_for_per_ray_use(hip_lib):
    """With the maxima of a reference grid passed in, a subset of the points evaluates to the same
    values as the full grid (the per-ray shading contract)."""
    from bhr_amd import disk_v2 as dv
    P = dv.DiskV2Params()
    cp = dv.pack_params(P, None, shear_seed=42, hotspot_seed=43)
    rg, pg = np.meshgrid(np.linspace(2.0, 10.0, 96), np.linspace(0, 2 * np.pi, 192, endpoint=False), indexing="ij")
    full, (m_sh, m_hs) = dv.evaluate(dv.F_TOTAL, cp, rg, phi=pg, return_max=True)
    assert m_sh > 0 and m_hs > 0
    sub = dv.evaluate(dv.F_TOTAL, cp, rg[10:20, 5:50], phi=pg[10:20, 5:50], norm_shear=m_sh, norm_hotspot=m_hs)
    np.testing.assert_allclose(sub, full[10:20, 5:50], rtol=1e-15, atol=0)


# ---- the field evaluator against the oracle's restatement: sizes, term counts, the max reduction ---------------
FIELD_TOL = dict(rtol=2e-14, atol=1e-15)          # fields 0..9, as against the tables
MOD_TOL = dict(rtol=1e-12, atol=1e-13)            # modulations 10..13
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 70001]  # empty, one lane, around a wave, around a block, 274 blocks + 1 lane


def _points(P, n_max=70001):
    """r, z, phi of n_max points; the first ones are the edges: r exactly r_in and r_out, one ulp either side of each,
    r = 0, and angles of +-1e3; the rest is spread over 0.3 r_in .. 1.3 r_out, |z| <= 1.3 H and angles in [-40, 40]."""
    rng = np.random.default_rng(11)
    r = rng.uniform(0.3 * P.r_in, 1.3 * P.r_out, n_max)
    phi = rng.uniform(-40.0, 40.0, n_max)
    edge = [P.r_in, P.r_out, np.nextafter(P.r_in, 0), np.nextafter(P.r_in, 99), np.nextafter(P.r_out, 0),
            np.nextafter(P.r_out, 99), 0.0, 0.5 * (P.r_in + P.r_out), 0.7 * P.r_out]
    r[:len(edge)] = edge
    phi[:len(edge)] = [1e3, -1e3, 0.0, 1e3, -1e3, 0.3, 1.0, 1e3, -1e3]
    h = P.h0 * np.maximum(r, P.r_in) * (np.maximum(r, P.r_in) / P.r_in) ** P.beta_h
    z = rng.uniform(-1.3, 1.3, n_max) * h
    z[:4] = [0.0, h[1], -h[2], np.nextafter(h[3], 99)]
    return r, z, phi


def _oracle_modulations(oracle, cp, r, phi):
    """F_mode, F_shear, F_hotspot, F_total as the reference defines them on an array (each signed sum divided by its
    maximum over that array), from the oracle's raw sums; plus the two maxima."""
    from bhr_amd import disk_v2 as dv
    raw_s, raw_h = oracle.dv2_eval(cp, dv.F_SHEAR, r, None, phi), oracle.dv2_eval(cp, dv.F_HOTSPOT, r, None, phi)
    m_s, m_h = (float(np.abs(a).max()) if a.size else 0.0 for a in (raw_s, raw_h))
    inside = oracle.dv2_eval(cp, dv.F_W_R, r) > 0
    eps = np.finfo(np.float64).eps
    f_s = np.where(inside, 1.0 + cp.shear_strength * (raw_s / m_s if m_s > eps else 0.0 * raw_s), 1.0)
    f_h = np.where(inside, 1.0 + cp.hotspot_strength * (raw_h / m_h if m_h > eps else 0.0 * raw_h), 1.0)
    f_m = oracle.dv2_eval(cp, dv.F_MODE, r, None, phi)
    return {dv.F_MODE: f_m, dv.F_SHEAR: f_s, dv.F_HOTSPOT: f_h, dv.F_TOTAL: np.where(inside, f_m * f_s * f_h, 1.0)}, (m_s, m_h)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["default", "alt", "sharp"])
def test_evaluator_matches_oracle_at_every_size(which, oracle, hip_lib):
    """Every field id at n = 0, 1, around a wave (63..65), around a block (255..257) and 70001 (a partial last block
    whose single lane is point 70000), on points that include both radii exactly and one ulp either side, r = 0 and
    phi = +-1e3.  "sharp" is the second set with edge_softness = 0."""
    from bhr_amd import disk_v2 as dv
    import disk_v2_sets as sets
    P, sp = sets.make(which)
    cp = dv.pack_params(P, sp, shear_seed=42, hotspot_seed=43)
    R, Z, PHI = _points(P)
    for n in SIZES:
        r, z, phi = R[:n], Z[:n], PHI[:n]
        for f in range(dv.F_MODE):
            got = dv.evaluate(f, cp, r, z=z)
            assert got.shape == (n,)
            np.testing.assert_allclose(got, oracle.dv2_eval(cp, f, r, z) if n else np.empty(0), err_msg=f"n={n} field {f}", **FIELD_TOL)
        want, (m_s, m_h) = _oracle_modulations(oracle, cp, r, phi) if n else ({f: np.empty(0) for f in range(10, 14)}, (0.0, 0.0))
        for f in (dv.F_MODE, dv.F_SHEAR, dv.F_HOTSPOT, dv.F_TOTAL):
            got, mx = dv.evaluate(f, cp, r, phi=phi, return_max=True)
            assert got.shape == (n,)
            np.testing.assert_allclose(got, want[f], err_msg=f"n={n} field {f}", **MOD_TOL)
            if f != dv.F_MODE:          # the device's own reduction of max |raw| (F_TOTAL: both sums)
                np.testing.assert_allclose(mx[0], m_h if f == dv.F_HOTSPOT else m_s, err_msg=f"n={n} field {f}", **MOD_TOL)
            if f == dv.F_TOTAL:
                np.testing.assert_allclose(mx[1], m_h, err_msg=f"n={n}", **MOD_TOL)
        if n == 257:
            # the fixed-norm path with the measured maxima passed in: the oracle's value, and a subset equals the array
            fixed = dv.evaluate(dv.F_TOTAL, cp, r, phi=phi, norm_shear=m_s, norm_hotspot=m_h)
            np.testing.assert_allclose(fixed, oracle.dv2_eval(cp, dv.F_TOTAL, r, None, phi, norm_shear=m_s, norm_hotspot=m_h), **MOD_TOL)
            full, (d_s, d_h) = dv.evaluate(dv.F_TOTAL, cp, r, phi=phi, return_max=True)
            sub = dv.evaluate(dv.F_TOTAL, cp, r[200:257], phi=phi[200:257], norm_shear=d_s, norm_hotspot=d_h)
            np.testing.assert_allclose(sub, full[200:257], rtol=1e-15, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_shear,n_hot", [(0, 0), (0, 32), (32, 0), (1, 1), (1, 32), (32, 32)])
def test_evaluator_term_counts(n_shear, n_hot, oracle, hip_lib):
    """0, 1 and BHR_DV2_MAX_TERMS shear components / hotspots, the counts written straight into the parameter block (the
    Python parameter class refuses 0).  With no terms the raw sum is identically 0, its maximum 0, and the factor
    exactly 1."""
    from bhr_amd import disk_v2 as dv
    import disk_v2_sets as sets
    P, sp = sets.make("alt")
    assert sp.shear_components == sp.hotspot_count == dv.MAX_TERMS == 32
    cp = dv.pack_params(P, sp, shear_seed=7, hotspot_seed=8)
    cp.shear_components, cp.hotspot_count = n_shear, n_hot
    R, _, PHI = _points(P, 300)
    want, (m_s, m_h) = _oracle_modulations(oracle, cp, R, PHI)
    for f in (dv.F_MODE, dv.F_SHEAR, dv.F_HOTSPOT, dv.F_TOTAL):
        got, mx = dv.evaluate(f, cp, R, phi=PHI, return_max=True)
        np.testing.assert_allclose(got, want[f], err_msg=f"field {f}", **MOD_TOL)
        if f == dv.F_SHEAR and n_shear == 0 or f == dv.F_HOTSPOT and n_hot == 0:
            assert mx[0] == 0.0 and (got == 1.0).all()
        if f == dv.F_TOTAL:
            np.testing.assert_allclose(mx, (m_s, m_h), **MOD_TOL)
            assert (mx[0] == 0.0) == (n_shear == 0) and (mx[1] == 0.0) == (n_hot == 0)
    fixed = dv.evaluate(dv.F_TOTAL, cp, R, phi=PHI, norm_shear=1.7, norm_hotspot=0.9)
    np.testing.assert_allclose(fixed, oracle.dv2_eval(cp, dv.F_TOTAL, R, None, PHI, norm_shear=1.7, norm_hotspot=0.9), **MOD_TOL)
    if n_shear == 0 and n_hot == 0:
        np.testing.assert_array_equal(fixed, dv.evaluate(dv.F_MODE, cp, R, phi=PHI))


MAX_CASES = {   # n, index of the largest |raw|: thread = index % 256, wave = thread // 64 of a 256-thread block
    "first": (600, 0),
    "last_lane_of_full_block": (512, 255),                 # wave 3, lane 63
    "last_of_partial_block": (256 + 200, 256 + 199),       # wave 3 of the last block, whose lanes 8..63 are past n
    "alone_in_last_wave": (512 + 192 + 1, 512 + 192),      # lane 0 of wave 3, every other lane of the wave past n
    "alone_in_second_wave": (512 + 64 + 1, 512 + 64),      # the same in wave 1, waves 2 and 3 wholly past n
    "all_negative": (600, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(MAX_CASES))
def test_evaluator_max_reduction(case, oracle, hip_lib):
    """max_out against np.abs(raw).max() of the oracle's raw sums, with the largest |raw| put where a reduction loses it:
    at index 0, in the last lane of a block, at index n - 1 of a partial last block, alone in a wave whose other lanes
    are past n (the last wave of the block and an earlier one), and with every raw value negative (the device orders
    the bit patterns of |raw|)."""
    from bhr_amd import disk_v2 as dv
    import disk_v2_sets as sets
    P, sp = sets.make("default")
    cp = dv.pack_params(P, sp, shear_seed=42, hotspot_seed=43)
    # candidates inside the disk, ranked by the oracle: one point where both |raw| sums are large, many where both are small
    rng = np.random.default_rng(3)
    r, phi = rng.uniform(2.5, 9.0, 20000), rng.uniform(0.0, 2 * np.pi, 20000)
    raw = {f: oracle.dv2_eval(cp, f, r, None, phi) for f in (dv.F_SHEAR, dv.F_HOTSPOT)}
    a_s, a_h = np.abs(raw[dv.F_SHEAR]), np.abs(raw[dv.F_HOTSPOT])
    if case == "all_negative":
        neg = (raw[dv.F_SHEAR] < 0) & (raw[dv.F_HOTSPOT] < 0)
        assert neg.sum() > 600
        idx = np.flatnonzero(neg)[:600]
        n = MAX_CASES[case][0]
    else:
        big = int(np.argmax(np.minimum(a_s / a_s.max(), a_h / a_h.max())))
        small = np.flatnonzero((a_s < 0.5 * a_s[big]) & (a_h < 0.5 * a_h[big]))
        n, where = MAX_CASES[case]
        assert small.size >= n
        idx = small[:n].copy()
        idx[where] = big
    rr, pp = r[idx], phi[idx]
    for f in (dv.F_SHEAR, dv.F_HOTSPOT, dv.F_TOTAL):
        _, mx = dv.evaluate(f, cp, rr, phi=pp, return_max=True)
        want = (a_h[idx].max() if f == dv.F_HOTSPOT else a_s[idx].max(), a_h[idx].max() if f == dv.F_TOTAL else 0.0)
        if case != "all_negative":
            assert want[0] == (a_h if f == dv.F_HOTSPOT else a_s)[big]
        np.testing.assert_allclose(mx, want, err_msg=f"{case} field {f}", **MOD_TOL)
        assert mx[0] > 0


@pytest.mark.gpu
def test_march_with_analytic_disk_source(hip_lib):
    """bhr_set_disk_source(BHR_DISK_V2): the in-kernel binary64 model equals (i) its host twin at sample
    points and (ii) a render from a fine texture baked with that twin, up to texture interpolation."""
    from bhr_amd import HipRenderer, scenes
    from bhr_amd import disk_v2 as dv
    P = dv.DiskV2Params(r_in=2.0, r_out=10.0)
    kw = dict(step_size=0.1, r_disk_inner=2.0, r_disk_outer=10.0, disk_tilt=10.0)
    sky = scenes.analytic_skybox(128, 256)
    n_r, n_phi = 768, 3072
    r = HipRenderer(256, 144, sky, np.zeros((n_r, n_phi, 4), dtype=np.float32), **kw)
    r.use_disk_v2(P, seed=42)
    cp, m_sh, m_hs, t_peak = r._dv2
    img_model = r.render([6, 0, 1.5], 90, skip_bloom=True)
    assert img_model.max() > 0.05 and np.isfinite(img_model).all()
    # bake: texel (i, j) sits at r = r_in + (i / n_r) span, phi = 2 pi j / n_phi (the lookup of _sample_disk)
    rr = 2.0 + (np.arange(n_r) / n_r) * 8.0
    pp = 2 * np.pi * np.arange(n_phi) / n_phi
    rg, pg = np.meshgrid(rr, pp, indexing="ij")
    tex = dv.disk_rgba(rg, pg, cp, m_sh, m_hs, t_peak, ctx=r._ctx)
    assert tex.shape == (n_r, n_phi, 4) and 0.0 < tex[..., 3].mean() < 1.0
    r.use_disk_v2(None)
    r.update_disk_texture(tex)
    img_tex = r.render([6, 0, 1.5], 90, skip_bloom=True)
    d = np.abs(img_model - img_tex)
    assert np.sqrt(np.mean(d ** 2)) < 2e-3 and np.quantile(d, 0.999) < 2e-2, (np.sqrt(np.mean(d ** 2)), d.max())
    # rotation: frame != 0 advects the analytic pattern with the model's own Omega(r)
    r.use_disk_v2(P, seed=42)
    moved = r.render([6, 0, 1.5], 90, frame=40, skip_bloom=True)
    assert np.abs(moved - img_model).max() > 1e-3
    r.close()
