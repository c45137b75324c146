"""Finite-thickness Disk V2 source of the march kernel (BHR_DISK_V2_VOLUME, docs/design_ad_v2.md 4.2-4.3).

The reference specifies this integrator but does not implement it (design_ad_v2.md 5.1 status table:
integrator.py "planned"), so there are no reference vectors: the kernel is checked against the oracle's
restatement of the same specification (whose Disk V2 fields ARE pinned by the reference's tables,
tests/test_oracle.py) and against the acceptance criteria the design lists for test_disk_v2_integrator.py /
test_disk_v2_advection.py: nothing off the disk, opacity grows with the path's optical depth, the grazing
gain thickens oblique views, more pieces per step converge, an axisymmetric disk does not change with time.
"""
import numpy as np
import pytest

from bhr_amd import scenes

pytestmark = pytest.mark.gpu

VIEWS = {
    "edge_on": dict(cam=[9.0, 0.0, 0.6], fov=70, tilt=0.0, frame=0),
    "tilted_later": dict(cam=[7.0, 2.0, 2.5], fov=80, tilt=12.0, frame=25),       # t_offset = 2.5: advected pattern
}
W, H = 192, 108


def _rmse(a, b):
    return np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2, axis=(0, 1)))


def _pair(oracle, view, math="strict", fast=False, **vol):
    from bhr_amd import HipRenderer, disk_v2 as dv
    P = dv.DiskV2Params()
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    kw = dict(step_size=0.1, r_disk_inner=P.r_in, r_disk_outer=P.r_out, disk_tilt=view["tilt"])
    hip = HipRenderer(W, H, sky, tex, math=math, **kw)
    hip.use_disk_v2(P, seed=42, volume=True, **vol)
    cp, m_s, m_h, t_peak = hip._dv2
    ora = oracle.OracleRenderer(W, H, sky, tex, fast=fast, **kw)
    ora.set_volume(cp, m_s, m_h, t_peak, vol.get("absorption", 4.0), vol.get("grazing_gain", 1.0), vol.get("substeps", 2))
    return hip, ora


@pytest.mark.parametrize("view", list(VIEWS))
def test_volume_matches_oracle_strict(view, oracle, hip_lib):
    from bhr_amd import _lib
    v = VIEWS[view]
    hip, ora = _pair(oracle, v, substeps=3)
    try:
        hip.render_async(v["cam"], v["fov"], frame=v["frame"], skip_bloom=True)
        bg, disk = hip.read_layer(_lib.LAYER_BG), hip.read_layer(_lib.LAYER_DISK)
        rbg, rdisk = (x.transpose(1, 0, 2) for x in ora.march(v["cam"], v["fov"], frame=v["frame"]))
    finally:
        ora.set_volume(None)
    assert disk.max() > 0.3 and (disk.sum(axis=2) > 0).mean() > 0.1          # the disk is really in view
    # identical ray paths (strict arithmetic); the model runs in binary64 on both sides, the per-sample
    # g-factor transcendentals differ by <= 2 ulp (ocml vs glibc) and accumulate over tens of samples
    for name, a, b in (("bg", bg, rbg), ("disk", disk, rdisk)):
        assert (_rmse(a, b) <= 1e-5).all(), f"{view}/{name}: RMSE {_rmse(a, b)}"
        assert np.abs(a - b).max() <= 2e-4, f"{view}/{name}: max {np.abs(a - b).max()}"
    assert hip.counters()["ray_steps"] == ora.last_total_steps
    hip.close()


# ---- where the bounding-slab cull of volume_segment (csrc/march_device.h) can bite --------------------------------
# The kernel skips a chord whose two ends lie outside a slab derived in bhr_set_disk_source (|zeta| <= max H, r_in <= |p|,
# |p| <= sqrt(r_out^2 + max H^2)); the oracle samples every chord.  96 x 54 frames (the last 8-row tile is partial)
# unless a case names its own size.
THICK = dict(h0=0.25, beta_h=0.3)            # flares outwards: H(r_out) = 4.05 is the maximum
INWARD = dict(h0=0.25, beta_h=-1.5)          # H(r) = h0 r_in (r / r_in)^-0.5: H(r_in) = 0.5 is the maximum, H(r_out) = 0.22
CAM0, CAM60 = dict(cam=[9.0, 0.0, 0.6], fov=70, tilt=0.0), dict(cam=[7.0, 2.0, 2.5], fov=80, tilt=60.0)
ABOVE0 = dict(cam=[8.0, 0.0, 6.0], fov=70, tilt=0.0)   # the thick disk from outside its flare: CAM0 sits inside it (H(9) = 3.5)
CULL_CASES = {
    "thick_tilt0": dict(params=THICK, **ABOVE0),
    "thick_tilt60": dict(params=THICK, **CAM60),
    "inward_tilt0": dict(params=INWARD, **CAM0),
    "inward_tilt60": dict(params=INWARD, **CAM60),
    "camera_inside_slab": dict(params=THICK, cam=[6.0, 0.0, 0.02], fov=70, tilt=0.0),     # the first chord starts in the volume
    "camera_on_axis": dict(params=THICK, cam=[0.0, 0.0, 9.0], fov=90, tilt=0.0),          # down the pole
    "sharp_edge_on": dict(params=dict(edge_softness=0.0), cam=[12.0, 0.0, 0.05], fov=70, tilt=0.0),   # density up to r_out
    "substeps1": dict(params=THICK, substeps=1, **ABOVE0),
    "substeps16": dict(params=THICK, substeps=16, **ABOVE0),
    "absorption50": dict(params=THICK, absorption=50.0, **ABOVE0),                          # rays stop at BHR_VOLUME_OPAQUE
    # One row of 16384 rays in the disk plane, 2e-4 apart, at step_size 0.5: chords 1.6 long near r_out, so that among the
    # ~80 rays tangent within 0.016 below r_out some have a chord whose two ends lie beyond the slab's outer radius
    # (10.0146) while its middle, where the single sample is taken, lies inside r_out -- in the sharp-edged disk, where the
    # density there is 0.2.  The cull of the parent commit read the ends alone and dropped those samples (70 pixels, up to
    # 1.9e-2; found with the cull restated inside the oracle); volume_segment now allows for half the chord.
    "coarse_step_tangent": dict(params=dict(edge_softness=0.0), cam=[12.2, 0.0, 0.0], fov=float(np.degrees(2 * np.arctan(1e-4))),
                                tilt=0.0, size=(16384, 1), step=0.5, substeps=1, absorption=1.0),   # Ca = 1: the hot inner disk shows through
}
# Measured (MI355X), largest per-channel RMSE / max |difference|:   BG                   DISK
#   thick_tilt0          2.5e-07 / 6.1e-06   3.4e-08 / 2.4e-07     thick_tilt60         1.1e-07 / 2.0e-06   3.3e-08 / 1.5e-07
#   inward_tilt0         5.0e-07 / 6.1e-06   2.3e-08 / 1.8e-07     inward_tilt60        5.7e-07 / 5.8e-06   2.2e-08 / 2.4e-07
#   camera_inside_slab   3.5e-09 / 9.8e-08   3.7e-08 / 2.4e-07     camera_on_axis       2.9e-07 / 5.3e-06   2.9e-08 / 2.4e-07
#   sharp_edge_on        6.3e-07 / 6.1e-06   7.9e-09 / 1.8e-07     substeps1            2.5e-07 / 6.1e-06   3.6e-08 / 2.4e-07
#   substeps16           2.5e-07 / 6.1e-06   3.4e-08 / 2.4e-07     absorption50         2.1e-07 / 6.1e-06   2.8e-08 / 1.8e-07
#   coarse_step_tangent  7.8e-08 / 2.8e-06   1.3e-08 / 1.2e-07     (the parent commit's cull: see the mutation note in the case)


@pytest.mark.parametrize("case", list(CULL_CASES))
def test_volume_cull_matches_oracle_strict(case, oracle, hip_lib):
    from bhr_amd import HipRenderer, _lib, disk_v2 as dv
    c = CULL_CASES[case]
    P = dv.DiskV2Params(**c["params"])
    vol = dict(substeps=c.get("substeps", 3), absorption=c.get("absorption", 4.0), grazing_gain=1.0)
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    kw = dict(step_size=c.get("step", 0.1), r_disk_inner=P.r_in, r_disk_outer=P.r_out, disk_tilt=c["tilt"])
    CULL_W, CULL_H = c.get("size", (96, 54))
    hip = HipRenderer(CULL_W, CULL_H, sky, tex, math="strict", **kw)
    hip.use_disk_v2(P, seed=42, volume=True, **vol)
    cp, m_s, m_h, t_peak = hip._dv2
    ora = oracle.OracleRenderer(CULL_W, CULL_H, sky, tex, **kw)
    ora.set_volume(cp, m_s, m_h, t_peak, vol["absorption"], vol["grazing_gain"], vol["substeps"])
    try:
        hip.render_async(c["cam"], c["fov"], frame=25, skip_bloom=True)
        bg, disk = hip.read_layer(_lib.LAYER_BG), hip.read_layer(_lib.LAYER_DISK)
        rbg, rdisk = (x.transpose(1, 0, 2) for x in ora.march(c["cam"], c["fov"], frame=25))
    finally:
        ora.set_volume(None)
    assert rdisk.max() > 0.3 and (rdisk.sum(axis=2) > 0).mean() > 0.1          # the disk is really in view
    for name, a, b in (("bg", bg, rbg), ("disk", disk, rdisk)):
        e, m = _rmse(a, b), float(np.abs(a - b).max())
        print(f"\n[{case} {name}] RMSE {e.max():.3g} max {m:.3g}")
        assert (e <= 1e-5).all(), f"{case}/{name}: RMSE {e}"
        assert m <= 2e-4, f"{case}/{name}: max {m} at {np.unravel_index(np.abs(a - b).argmax(), a.shape)}"
    assert hip.counters()["ray_steps"] == ora.last_total_steps
    hip.close()


def test_volume_fast_math_against_binary64(oracle, hip_lib):
    from bhr_amd import _lib
    v = VIEWS["edge_on"]
    hip, ora = _pair(oracle, v, math="fast", fast="f64")
    try:
        hip.render_async(v["cam"], v["fov"], skip_bloom=True)
        disk = hip.read_layer(_lib.LAYER_DISK)
        rdisk = ora.march(v["cam"], v["fov"])[1].transpose(1, 0, 2)
    finally:
        ora.set_volume(None)
    assert (_rmse(disk, rdisk) <= 1e-4).all(), _rmse(disk, rdisk)
    hip.close()


def _render(view, **vol):
    from bhr_amd import HipRenderer, _lib, disk_v2 as dv
    P = vol.pop("params", None) or dv.DiskV2Params()
    sp = vol.pop("structure", None)
    frame = vol.pop("frame", view["frame"])
    hip = HipRenderer(W, H, scenes.analytic_skybox(), scenes.noisy_disk(), step_size=0.1, r_disk_inner=P.r_in,
                      r_disk_outer=P.r_out, disk_tilt=view["tilt"])
    hip.use_disk_v2(P, sp, seed=42, volume=True, **vol)
    hip.render_async(view["cam"], view["fov"], frame=frame, skip_bloom=True)
    out = hip.read_layer(_lib.LAYER_BG), hip.read_layer(_lib.LAYER_DISK)
    hip.close()
    return out


def test_integrator_acceptance_criteria(hip_lib):
    from bhr_amd import HipRenderer, _lib
    v = VIEWS["edge_on"]
    # no absorption, no emission: the disk layer is exactly empty and the sky is untouched
    bg0, disk0 = _render(v, absorption=0.0)
    assert disk0.max() == 0.0
    plain = HipRenderer(W, H, scenes.analytic_skybox(), np.zeros((32, 64, 4), np.float32), step_size=0.1,
                        r_disk_inner=2.0, r_disk_outer=10.0)
    plain.render_async(v["cam"], v["fov"], skip_bloom=True)
    np.testing.assert_array_equal(bg0, plain.read_layer(_lib.LAYER_BG))
    plain.close()
    # the longer the optical path, the less sky comes through: transmission falls monotonically with Ca
    sky_through = [(_render(v, absorption=ca)[0]).sum() for ca in (0.5, 2.0, 8.0)]
    assert sky_through[0] > sky_through[1] > sky_through[2] and sky_through[0] < bg0.sum()
    # grazing-angle gain: an edge-on view gets more opaque, and the gain only ever adds opacity
    flat, gained = _render(v, grazing_gain=0.0)[0], _render(v, grazing_gain=2.0)[0]
    assert gained.sum() < 0.98 * flat.sum() and (gained <= flat + 2e-4).all()      # 2e-4: rays stop at opacity 0.9999
    # more pieces per step converge
    ref = _render(v, substeps=16)[1]
    err = [np.abs(_render(v, substeps=n)[1] - ref).mean() for n in (1, 4, 8)]
    assert err[0] > err[1] > err[2] and err[2] < 0.25 * err[0]


def test_advection_needs_structure(hip_lib):
    """phi_adv = phi + t Omega(r): an axisymmetric disk (no modes, shear or hotspots) looks the same at every
    time, the structured one does not."""
    from bhr_amd import disk_v2 as dv
    v = VIEWS["tilted_later"]
    flat = dv.DiskV2StructureParams(mode1_strength=0.0, mode2_strength=0.0, shear_strength=0.0, hotspot_strength=0.0)
    a, b = _render(v, structure=flat, frame=0)[1], _render(v, structure=flat, frame=40)[1]
    assert np.abs(a - b).max() <= 1e-6
    a, b = _render(v, frame=0)[1], _render(v, frame=40)[1]
    assert np.abs(a - b).mean() > 1e-3


def test_volume_option_validation(hip_lib):
    from bhr_amd import HipRenderer, disk_v2 as dv
    r = HipRenderer(32, 18, scenes.analytic_skybox(), scenes.noisy_disk())
    for bad in (dict(absorption=-1.0), dict(grazing_gain=-0.5), dict(substeps=0), dict(substeps=17)):
        with pytest.raises(ValueError):
            r.use_disk_v2(dv.DiskV2Params(), volume=True, **bad)
    r.use_disk_v2(dv.DiskV2Params(), volume=True)
    r.use_disk_v2(None)                       # back to the texture
    r.close()
