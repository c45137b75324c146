"""The analytic Disk V2 surface source of the march (BHR_DISK_V2: march_tile_kernel<., 1>, disk_v2_rgba in
csrc/march_device.h) against the oracle's surface mode (oracle/bhr_oracle.c: dv2_surface_rgba), which is written from
the mapping's specification and pinned on the CPU by tests/test_oracle.py -- its fields by the reference package's
tables at two parameter sets, its colour mapping by a float32 NumPy restatement.

Strict arithmetic marches the oracle's ray paths bit for bit, the model runs in binary64 on both sides and the colour
mapping and g-factor in float32 with libm's transcendentals on one side and ocml's on the other; a ray composites a
handful of crossings.  The bars are the ones the finite-thickness source is held to (test_gpu_volume.py): per-channel
RMSE <= 1e-5 and max |difference| <= 2e-4, on the BG and DISK layers, and the same number of ray steps.

Measured (MI355X), largest per-channel RMSE / max |difference| over frames 0 and 25:
                                  BG RMSE / max          DISK RMSE / max
  default  edge_on   (both kernels)  4.7e-07 / 6.1e-06   2.4e-08 / 3.0e-07
  default  tilt35    (both kernels)  4.3e-07 / 6.1e-06   3.1e-08 / 3.6e-07
  default  below60   (both kernels)  4.0e-07 / 5.8e-06   3.3e-08 / 3.6e-07
  alt      edge_on   (both kernels)  6.4e-07 / 6.1e-06   1.6e-08 / 3.0e-07
  alt      tilt35    (both kernels)  4.6e-07 / 6.1e-06   2.3e-08 / 3.0e-07
  alt      below60   (both kernels)  4.0e-07 / 5.8e-06   2.3e-08 / 3.0e-07
  default  tilt35, gate 3.5..6       6.7e-07 / 6.1e-06   1.5e-08 / 2.4e-07
  fast     edge_on, DISK against the binary64 oracle     3.5e-06 / 2.2e-04   (bar: RMSE 1e-4)
With and without differentials the figures are the same to every digit shown; ray steps equal in every case.  The BG
difference is the sky sampler's (acos / atan2 of ocml against libm), as in the texture tests; the DISK layer is within
two f32 ulps of 1.
"""
import numpy as np
import pytest

from bhr_amd import scenes

pytestmark = pytest.mark.gpu

W, H = 96, 54                       # 54 rows: the last 8-row tile is partial
VIEWS = {
    "edge_on": dict(cam=[9.0, 0.0, 0.6], fov=70, tilt=0.0),
    "tilt35": dict(cam=[7.0, 2.0, 2.5], fov=80, tilt=35.0),
    "below60": dict(cam=[6.0, -3.0, -4.0], fov=90, tilt=60.0),        # from below the plane
}
FRAMES = (0, 25)                    # t_offset 0 and 2.5: the pattern advected by phi + t Omega(r)
RMSE_BAR, MAX_BAR = 1e-5, 2e-4


def _rmse(a, b):
    return np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2, axis=(0, 1)))


def _pair(oracle, which, tilt, math="strict", fast=False, gate=None):
    """A device renderer with the surface source of the named parameter set and the oracle in surface mode with the
    SAME constants (the device measures the normalisation maxima and the peak temperature on its reference grid)."""
    from bhr_amd import HipRenderer
    import disk_v2_sets as sets
    P, sp = sets.make(which)
    r_in, r_out = gate or (P.r_in, P.r_out)
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    # anti-aliasing on: a march then integrates the ray differentials unless a call skips them (the surface source
    # never reads the level they ask for)
    kw = dict(step_size=0.1, r_disk_inner=r_in, r_disk_outer=r_out, disk_tilt=tilt, anti_alias="lod_radius")
    hip = HipRenderer(W, H, sky, tex, math=math, **kw)
    hip.use_disk_v2(P, sp, seed=42)
    cp, m_s, m_h, t_peak = hip._dv2
    ora = oracle.OracleRenderer(W, H, sky, tex, fast=fast, **kw)
    ora.set_disk_v2_surface(cp, m_s, m_h, t_peak)
    return hip, ora


def _frames(hip, ora, v, frame, skip_diff):
    from bhr_amd import _lib
    hip.render_async(v["cam"], v["fov"], frame=frame, skip_bloom=True, skip_differentials=skip_diff)
    got = hip.read_layer(_lib.LAYER_BG), hip.read_layer(_lib.LAYER_DISK)
    want = tuple(x.transpose(1, 0, 2) for x in ora.march(v["cam"], v["fov"], frame=frame, skip_differentials=skip_diff))
    return got, want


def _check_strict(hip, ora, v, tag, skip_diff):
    disks = []
    for frame in FRAMES:
        (bg, disk), (rbg, rdisk) = _frames(hip, ora, v, frame, skip_diff)
        assert rdisk.max() > 0.3 and (rdisk.sum(axis=2) > 0).mean() > 0.1          # the disk is really in view
        for name, a, b in (("bg", bg, rbg), ("disk", disk, rdisk)):
            e, m = _rmse(a, b), float(np.abs(a - b).max())
            print(f"\n[{tag} frame {frame} {name}] RMSE {e.max():.3g} max {m:.3g}")
            assert (e <= RMSE_BAR).all(), f"{tag} frame {frame} {name}: RMSE {e}"
            assert m <= MAX_BAR, f"{tag} frame {frame} {name}: max {m} at {np.unravel_index(np.abs(a - b).argmax(), a.shape)}"
        assert hip.counters()["ray_steps"] == ora.last_total_steps
        disks.append(rdisk)
    assert np.abs(disks[0] - disks[1]).mean() > 1e-3                                # ... and the two frames differ


@pytest.mark.parametrize("skip_diff", [False, True], ids=["diff", "nodiff"])
@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("which", ["default", "alt"])
def test_surface_source_matches_oracle_strict(which, view, skip_diff, oracle, hip_lib):
    """Both parameter sets, the renderer's radii set to the model's; with and without ray differentials: two kernel
    instantiations, march_tile_kernel<true, 1> and <false, 1>."""
    v = VIEWS[view]
    hip, ora = _pair(oracle, which, v["tilt"])
    try:
        _check_strict(hip, ora, v, f"{which} {view} {'nodiff' if skip_diff else 'diff'}", skip_diff)
    finally:
        ora.set_disk_v2_surface(None)
        hip.close()


def test_surface_source_narrow_gate(oracle, hip_lib):
    """The renderer's radii strictly inside the model's: the march gates a crossing on the renderer's 3.5 <= r <= 6, the
    model its fields on its own 2 <= r <= 10 (and the g-factor's radial boost reads the renderer's).  Both must hold:
    nothing outside the narrow ring, and inside it the model's values, not ones rescaled to the ring."""
    from bhr_amd import HipRenderer, _lib
    import disk_v2_sets as sets
    v = VIEWS["tilt35"]
    hip, ora = _pair(oracle, "default", v["tilt"], gate=(3.5, 6.0))
    P, sp = sets.make("default")
    wide = HipRenderer(W, H, scenes.analytic_skybox(), scenes.noisy_disk(), step_size=0.1, r_disk_inner=P.r_in,
                       r_disk_outer=P.r_out, disk_tilt=v["tilt"], anti_alias="lod_radius")
    wide.use_disk_v2(P, sp, seed=42)
    try:
        _check_strict(hip, ora, v, "default tilt35 gate 3.5..6", False)
        hip.render_async(v["cam"], v["fov"], skip_bloom=True)
        wide.render_async(v["cam"], v["fov"], skip_bloom=True)
        lit_n = hip.read_layer(_lib.LAYER_DISK).sum(axis=2) > 0
        lit_w = wide.read_layer(_lib.LAYER_DISK).sum(axis=2) > 0
        assert (lit_w | ~lit_n).all() and 0.2 * lit_w.sum() < lit_n.sum() < 0.7 * lit_w.sum()
    finally:
        ora.set_disk_v2_surface(None)
        hip.close()
        wide.close()


def test_surface_source_fast_math_against_binary64(oracle, hip_lib):
    """math="fast" against the binary64 build of the oracle, at the bar the finite-thickness source's fast march has."""
    v = VIEWS["edge_on"]
    hip, ora = _pair(oracle, "default", v["tilt"], math="fast", fast="f64")
    try:
        (_, disk), (_, rdisk) = _frames(hip, ora, v, 0, False)
    finally:
        ora.set_disk_v2_surface(None)
        hip.close()
    assert rdisk.max() > 0.3 and (rdisk.sum(axis=2) > 0).mean() > 0.1
    print(f"\n[fast edge_on disk] RMSE {_rmse(disk, rdisk).max():.3g} max {np.abs(disk - rdisk).max():.3g}")
    assert (_rmse(disk, rdisk) <= 1e-4).all(), _rmse(disk, rdisk)
