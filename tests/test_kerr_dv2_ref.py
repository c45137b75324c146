"""tests/kerr_dv2_ref.py, the CPU reference of the Kerr march over the Disk V2 sources: its geometry, its colour mapping against
the oracle's, its frames at A = 0 against the oracle's strict Schwarzschild Disk V2 frames (the distances the device's spin-0 test
takes its bars from), and that its float32 and float64 runs agree on every ray's fate."""
import numpy as np
import pytest

import kerr_cases as KC
import kerr_dv2_cases as DC
import kerr_dv2_ref as D
import kerr_ref as K

KW = dict(step_size=KC.STEP, r_max=KC.R_MAX, r_disk_inner=KC.R_INNER, r_disk_outer=KC.R_OUTER, disk_tilt=0.0, anti_alias="disabled")


def test_on_the_plane_varpi_is_the_boyer_lindquist_hit_radius_and_at_spin_zero_the_cylindrical_one():
    rng = np.random.default_rng(3)
    x = rng.uniform(-12.0, 12.0, size=(4096, 3))
    for A in (0.6, -0.9, 0.998):
        a = A * K.M
        plane = x.copy()
        plane[:, 2] = 0.0
        plane = plane[(plane[:, :2] ** 2).sum(-1) > a * a + 1e-3]      # outside the ring's disk, where the plane is r > 0
        w, zeta, phi = D.cylinder(plane, a)
        assert np.allclose(w, np.sqrt((plane[:, :2] ** 2).sum(-1) - a * a), rtol=1e-12, atol=1e-12)
        assert (zeta == 0).all() and np.array_equal(phi, np.arctan2(plane[:, 1], plane[:, 0]))
        # off the plane: r^2 = varpi^2 + zeta^2 with r the Kerr-Schild radius, and varpi = r sin(theta) of z = r cos(theta)
        w, zeta, _ = D.cylinder(x, a)
        r = K.ks_radius(x, a)
        assert np.allclose(w * w + zeta * zeta, r * r, rtol=1e-12)
        assert np.allclose(w, r * np.sqrt(np.maximum(1.0 - (x[:, 2] / r) ** 2, 0.0)), rtol=1e-9, atol=1e-9)
        # the Euclidean distance and r differ by no more than |a| (what the device's cull leans on)
        d = np.sqrt((x * x).sum(-1))
        assert (r <= d * (1 + 1e-15)).all() and (d * d <= r * r + a * a + 1e-9).all()
    w, zeta, _ = D.cylinder(x, 0.0)
    assert np.allclose(w, np.sqrt((x[:, :2] ** 2).sum(-1)), rtol=1e-13) and np.array_equal(zeta, x[:, 2])


@pytest.mark.parametrize("t_offset", [0.0, 7.3])
def test_surface_mapping_is_the_oracles_at_spin_zero(t_offset, oracle):
    """kerr_dv2_ref.surface_rgba (fields from oracle.dv2_eval, the colour restated in NumPy) against the oracle's own surface
    mapping, which restates csrc/march_device.h: disk_v2_rgba.  The oracle's colour runs in f32: 1e-6 is a few of its ulps."""
    mdl = DC.model()
    rng = np.random.default_rng(5)
    rad, phi = rng.uniform(1.5, 11.0, 4096), rng.uniform(-np.pi, np.pi, 4096)
    xy = np.stack([rad * np.cos(phi), rad * np.sin(phi)], axis=-1).astype(np.float32)
    want = oracle.probe_dv2_rgba(mdl.cp, (mdl.norm_shear, mdl.norm_hotspot), mdl.t_peak, xy.astype(np.float64), t_offset)
    for dtype, tol in ((np.float32, 1e-6), (np.float64, 1e-6)):
        rgb, alpha = D.surface_rgba(mdl, xy[:, 0].astype(dtype), xy[:, 1].astype(dtype), 0.0, t_offset)
        assert rgb.dtype == dtype and alpha.dtype == dtype
        assert np.abs(rgb - want[:, :3]).max() <= tol and np.abs(alpha - want[:, 3]).max() <= tol
    assert want[:, 3].max() > 0.5 and want[:, :3].max() > 0.5 and (want[rad > 10.0, 3] == 0).all()


def _oracle_frame(oracle, kind, view):
    sky, tex = KC.scene()
    mdl = DC.model()
    o = oracle.OracleRenderer(KC.W, KC.H, sky, tex, **KW)
    if kind == "surface":
        o.set_disk_v2_surface(mdl.cp, mdl.norm_shear, mdl.norm_hotspot, mdl.t_peak)
    else:
        o.set_volume(mdl.cp, mdl.norm_shear, mdl.norm_hotspot, mdl.t_peak, 4.0, 1.0, DC.SUBSTEPS)
    try:
        _, img, disk, _ = o.render(list(view), KC.FOV, skip_differentials=True, skip_bloom=True, parts=True)
    finally:
        o.set_volume(None)
        o.set_disk_v2_surface(None)
    out = dict(bg=img.transpose(1, 0, 2), disk=disk.transpose(1, 0, 2))
    out["final"] = np.clip(out["bg"] + out["disk"], 0, 1)
    return out


@pytest.mark.parametrize("view", KC.VIEWS, ids=lambda v: f"pov{v[0]:g}_{v[1]:g}")
@pytest.mark.parametrize("kind", ["surface", "volume"])
def test_spin_zero_against_the_oracles_strict_disk_v2_frames(kind, view, oracle):
    """kerr_dv2_ref in binary64 at A = 0 against the oracle's strict Schwarzschild frame of the same model (kerr_dv2_cases.ORACLE_DISTANCE
    says what differs), over the pixels whose ray reaches the sky in both or in neither; the distances are the recorded ones."""
    ora = _oracle_frame(oracle, kind, view)
    r64 = DC.reference(DC.Case(kind, 0.0, view))
    same = (ora["bg"].max(axis=2) > 0) == (r64["fate"] == 1)
    got = KC.distance(ora, r64, same)
    print(f"{kind} {view}: fate differs on {float((~same).mean()):.3%}; kerr_dv2_ref f64 vs oracle strict {got}")
    assert float((~same).mean()) <= 0.005 and r64["disk"].max() > 0.5
    for layer, want in DC.ORACLE_DISTANCE[(kind, view)].items():
        assert got[layer] == pytest.approx(want, rel=0.02), layer       # the recorded figure, to its digits


@pytest.mark.parametrize("case", DC.SURFACE, ids=lambda c: c.id)
def test_float32_and_float64_marches_agree_on_every_fate(case):
    """What leaves the 0.5 % of a frame the device test may drop to the device alone."""
    d32, share = DC.float32_distance(case)
    print(f"{case.id}: float32 vs float64 {d32}, fate / crossing count differs on {share:.3%}")
    assert share == 0.0
    assert all(v < 1e-3 for v in d32.values())


def test_volume_reference_properties():
    """No absorption, no disk; more absorption, more opacity; the thin default disk seen from above its plane leaves the far sky alone."""
    sky, _ = KC.scene()
    cam = K.build_camera(list(KC.VIEWS[0]), KC.FOV, 24, 16, KC.R_MAX)
    kw = dict(h_base=KC.STEP, r_inner=KC.R_INNER, r_outer=KC.R_OUTER, substeps=2)
    none = D.render_volume(cam, 0.9, sky, DC.model(), absorption=0.0, **kw)
    thin = D.render_volume(cam, 0.9, sky, DC.model(), absorption=1.0, **kw)
    thick = D.render_volume(cam, 0.9, sky, DC.model(), absorption=8.0, **kw)
    assert none["disk"].max() == 0.0 and thin["disk"].max() > 0.0
    lit = thin["disk"].sum(axis=2) > 0
    assert 0.05 < lit.mean() < 0.95
    assert np.array_equal(none["bg"][~lit], thin["bg"][~lit])               # a ray that met no gas shows the sky untouched
    esc = (none["fate"] == 1) & lit
    assert (thick["bg"][esc].sum(axis=1) <= thin["bg"][esc].sum(axis=1) + 1e-12).all() and thick["bg"][esc].sum() < thin["bg"][esc].sum()
