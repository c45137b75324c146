"""The Kerr march over the analytic Disk V2 sources on the device (bhr_set_kerr_disk_source; csrc/ray_kerr_dv2.h) against its CPU
reference tests/kerr_dv2_ref.py in binary64 -- surface and volume, the cull of chords, ragged frames, supersampling, advection --
against the context's own strict Schwarzschild Disk V2 frames at spin 0, and its state: refusals, the way back to the texture,
resources.

Bars: test_gpu_kerr.py's rule.  Per layer max(twice what the float32 run of the reference keeps from its float64 run, 1e-4) as
RMSE over the pixels whose fate and crossing count on the device are the float64 reference's; at most 0.5 % of a frame may be left
out.  The device's fates and crossing counts are read from a probe frame of the TEXTURE Kerr march on the same camera -- a white
sky, constant opacity 1/2 per crossing: the steps and the crossing test are the same code as under a Disk V2 source.  The float32
and float64 references agree on every fate (tests/test_kerr_dv2_ref.py), so what is left out is the device's alone.  The volume has
no crossings: its frames are compared over the pixels of equal sky / no-sky fate."""
import functools

import numpy as np
import pytest

import kerr_cases as KC
import kerr_dv2_cases as DC
from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

BAR_FLOOR = 1e-4
FATE_SHARE = 0.005
PROBE_ALPHA = float(1.0 - 0.5 ** (1.0 / 6.0))        # disk_alpha = 1 - (1 - alpha)^6 = 1/2
SPEED = 0.1                                           # disk_rotation_speed: t_offset = frame * SPEED


def _kw(case):
    return dict(step_size=KC.STEP, r_max=KC.R_MAX, r_disk_inner=case.r_inner, r_disk_outer=KC.R_OUTER, disk_tilt=0.0, anti_alias="disabled",
                disk_rotation_speed=SPEED)


def _probe_scene():
    sky = np.ones((16, 32, 3), dtype=np.float32)
    tex = np.ones((8, 16, 4), dtype=np.float32)
    tex[..., 3] = PROBE_ALPHA
    return sky, tex


def _layers(r, case):
    from bhr_amd import _lib
    r.render_async(list(case.view), case.fov, frame=int(round(case.t_offset / SPEED)), skip_bloom=True)
    return dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), final=r.read_layer(_lib.LAYER_FINAL))


def _renderer(case, scene=None, supersample=1, width=None, height=None, kerr=True):
    from bhr_amd import HipRenderer
    sky, tex = scene or KC.scene()
    r = HipRenderer(width or case.width, height or case.height, sky, tex, math="strict", supersample=supersample, **_kw(case))
    if kerr:
        r.set_spin(case.A, force_kerr=(case.A == 0.0))
        if case.redshift == "exact":
            r.set_redshift("exact")
    return r


def _use(r, case, kerr=True):
    p, sp = DC.params(case)
    (r.use_kerr_disk_v2 if kerr else r.use_disk_v2)(p, sp, seed=42, volume=case.kind == "volume", substeps=DC.SUBSTEPS)


@functools.lru_cache(maxsize=None)
def _device(case, supersample=1, width=None, height=None):
    """Layers and counters of one device frame under the Kerr Disk V2 source of the case."""
    r = _renderer(case, supersample=supersample, width=width, height=height)
    _use(r, case)
    out = dict(frame=_layers(r, case), counters=r.counters())
    r.close()
    return out


@functools.lru_cache(maxsize=None)
def _probe(A, view, fov, r_inner, width, height, kerr=True):
    """(reached the sky, crossings of such a ray or -1, a captured ray crossed the disk) of the texture march's probe frame."""
    case = DC.Case("surface", A, view, fov=fov, r_inner=r_inner, width=width, height=height)
    r = _renderer(case, scene=_probe_scene(), kerr=kerr)
    probe = _layers(r, case)
    r.close()
    bg = probe["bg"][..., 0].astype(np.float64)
    sky = bg > 0
    n = np.where(sky, np.rint(-np.log2(np.where(sky, bg, 1.0))), -1).astype(np.int64)
    return sky, n, probe["disk"].max(axis=2) > 0


def _probe_of(case, kerr=True):
    return _probe(case.A, case.view, case.fov, case.r_inner, case.width, case.height, kerr)


def _same_as_reference(case, ref):
    sky, n, dark_hit = _probe_of(case)
    ref_sky = ref["fate"] == 1
    same = sky == ref_sky
    if case.kind == "surface":
        same &= np.where(sky & ref_sky, n == ref["n_hits"], True)
        same &= np.where(~sky & ~ref_sky, dark_hit == (ref["n_hits"] > 0), True)
    return same


def _against_reference(case):
    r64 = DC.reference(case, np.float64)
    d32, share32 = DC.float32_distance(case)
    dev = _device(case)
    same = _same_as_reference(case, r64)
    got = KC.distance(dev["frame"], r64, same)
    share = float((~same).mean())
    print(f"{case.id}: fate / crossing count differs on {share:.3%} (float32 reference: {share32:.3%}); device vs f64 {got}; float32 reference vs f64 {d32}")
    assert share <= FATE_SHARE
    for layer in ("bg", "disk", "final"):
        bar = max(2.0 * d32[layer], BAR_FLOOR)
        assert got[layer] <= bar, f"{layer}: RMSE {got[layer]:.3g} over the bar {bar:.3g}"
    return dev, r64


# ---- 1, 2, 4, 5: against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.SURFACE + DC.SURFACE_EXACT + [DC.SURFACE_LATER], ids=lambda c: c.id)
def test_surface_against_the_reference(case, hip_lib):
    dev, r64 = _against_reference(case)
    assert dev["frame"]["disk"].max() > 0.1 and dev["frame"]["bg"].max() > 0
    assert dev["counters"]["rays"] == case.width * case.height


@pytest.mark.parametrize("case", DC.VOLUME + [DC.VOLUME_THICK], ids=lambda c: c.id)
def test_volume_against_the_reference(case, hip_lib):
    dev, r64 = _against_reference(case)
    assert dev["frame"]["disk"].max() > 0.1 and dev["frame"]["bg"].max() > 0
    steps, want = int(dev["counters"]["ray_steps"]), int(DC.reference(case, np.float32)["steps"].sum())
    assert abs(steps - want) <= 2e-4 * want                      # the march is the Kerr march's: the chords change no ray


@pytest.mark.parametrize("case", DC.CULL, ids=lambda c: c.id)
def test_the_cull_drops_no_chord_the_reference_samples(case, hip_lib):
    """The equatorial camera looks along the slab, the close-in one sits inside the volume's radii next to a fast hole, where the
    Kerr-Schild radius and the Euclidean distance differ most: the reference samples every chord."""
    dev, r64 = _against_reference(case)
    assert (r64["disk"].sum(axis=2) > 0).mean() > 0.05 and dev["frame"]["disk"].max() > 0.1


@pytest.mark.parametrize("case", DC.RAGGED, ids=lambda c: c.id)
def test_ragged_frames(case, hip_lib):
    dev, r64 = _against_reference(case)
    assert dev["frame"]["bg"].shape == (case.height, case.width, 3) and np.isfinite(dev["frame"]["final"]).all()


# ---- 3: spin 0 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", KC.VIEWS, ids=lambda v: f"pov{v[0]:g}_{v[1]:g}")
@pytest.mark.parametrize("kind", ["surface", "volume"])
def test_forced_kerr_at_spin_zero_is_the_strict_disk_v2_frame(kind, view, hip_lib):
    """The Kerr Disk V2 kernels at A = 0 against the same configuration's strict Schwarzschild use_disk_v2 frame, within twice what
    kerr_dv2_ref (f64, A = 0) keeps from the oracle's strict frame (kerr_dv2_cases.ORACLE_DISTANCE, pinned by the CPU test)."""
    case = DC.Case(kind, 0.0, view)
    kerr = _device(case)["frame"]
    r = _renderer(case, kerr=False)
    _use(r, case, kerr=False)
    strict = _layers(r, case)
    r.close()
    s_sky, s_n, s_dark = _probe_of(case, kerr=False)
    k_sky, k_n, k_dark = _probe_of(case)
    same = (s_sky == k_sky) if kind == "volume" else (s_sky == k_sky) & (s_n == k_n) & (s_dark == k_dark)
    got = KC.distance(kerr, strict, same)
    share = float((~same).mean())
    print(f"{kind} {view}: forced Kerr vs strict: fate / crossing count differs on {share:.3%}; distance {got}; recorded kerr_dv2_ref f64 vs oracle "
          f"{DC.ORACLE_DISTANCE[(kind, view)]}")
    assert share <= FATE_SHARE and strict["disk"].max() > 0.1
    for layer in ("bg", "disk", "final"):
        assert got[layer] <= 2.0 * DC.ORACLE_DISTANCE[(kind, view)][layer], f"{layer}: RMSE {got[layer]:.3g}"


# ---- 6: supersampling -----------------------------------------------------------------------------------------------------------------
def _ulp_close(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


@pytest.mark.parametrize("kind", ["surface", "volume"])
def test_supersampled_frame_is_the_box_filter_of_the_fine_frame(kind, hip_lib):
    """supersample = 2 at 48 x 32 against the box filter of the 96 x 64 frame of the same configuration, within 1 ulp per value;
    the same rays, so the same steps (test_gpu_kerr.py does it for the texture)."""
    case = DC.Case(kind, 0.6, KC.VIEWS[0])
    ss = _device(case, supersample=2, width=KC.W // 2, height=KC.H // 2)
    fine = _device(case)
    for layer in ("bg", "disk"):
        want = box_resolve(fine["frame"][layer], 2)
        bad = int((~_ulp_close(ss["frame"][layer], want)).any(axis=2).sum())
        assert bad == 0, f"{layer}: {bad} pixels more than 1 ulp from the box filter of the 96 x 64 frame"
    assert ss["counters"]["rays"] == KC.W * KC.H and ss["counters"]["ray_steps"] == fine["counters"]["ray_steps"]
    assert ss["frame"]["disk"].max() > 0


# ---- 7: advection -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["surface", "volume"])
def test_the_pattern_turns_and_an_axisymmetric_disk_does_not(kind, hip_lib):
    base = DC.Case(kind, 0.6, KC.VIEWS[0])
    later = base._replace(t_offset=float(np.float32(73 * SPEED)))
    a, b = _device(base)["frame"], _device(later)["frame"]
    assert np.abs(a["disk"] - b["disk"]).max() > 1e-3                     # the default structure is advected
    flat = base._replace(structure=False)
    a, b = _device(flat)["frame"], _device(flat._replace(t_offset=later.t_offset))["frame"]
    for layer in ("bg", "disk"):
        assert np.abs(a[layer] - b[layer]).max() <= 1e-6, layer
    assert a["disk"].max() > 0.1


# ---- 8: state -------------------------------------------------------------------------------------------------------------------------
def test_state_and_refusals(hip_lib):
    import ctypes as C
    from bhr_amd import _lib
    from bhr_amd.disk_v2 import DiskV2Params
    case = DC.Case("surface", 0.5, (6.0, 0.0, 0.5), width=32, height=16)
    view, P = list(case.view), DiskV2Params()

    def refused(fn, kind, *words):
        with pytest.raises(kind) as e:
            fn()
        msg = str(e.value).lower()
        assert all(w in msg for w in words), msg

    def source(r, src, cp=None, norms=(1.0, 1.0, 1.0)):
        return lambda: _lib.check(r._lib.bhr_set_kerr_disk_source(r._ctx, src, C.byref(cp) if cp is not None else None, *norms))

    # the Kerr source without the Kerr march: BHR_ERR_STATE, like bhr_set_kerr_anti_alias
    r = _renderer(case, kerr=False)
    refused(lambda: r.use_kerr_disk_v2(P), AssertionError, "kerr disk v2 source", "without the kerr march")
    assert r._lib.bhr_set_kerr_disk_source(r._ctx, 1, None, 1.0, 1.0, 1.0) == _lib.BHR_ERR_STATE
    r.use_kerr_disk_v2(None)                               # the texture is always accepted
    r.close()

    # the same validation as bhr_set_disk_source
    r = _renderer(case)
    r.use_kerr_disk_v2(P)
    from bhr_amd import disk_v2 as dv
    cp = dv.pack_params(P)
    refused(source(r, 7, cp), ValueError, "bhr_set_kerr_disk_source", "source 7")
    refused(source(r, 1, None), ValueError, "bhr_set_kerr_disk_source", "needs parameters")
    refused(source(r, 1, cp, (0.0, 1.0, 1.0)), ValueError, "bhr_set_kerr_disk_source", "positive normalisation")
    bad = dv.pack_params(P)
    bad.r_out = 1.0
    refused(source(r, 2, bad), ValueError, "bhr_set_kerr_disk_source", "inconsistent")
    assert r.kerr_disk_model == "v2"
    # while the source is set: spin 0 without the force, the Kerr anti-aliasing, the Kerr camera, map builds, shutter frames
    refused(lambda: r.set_spin(0.0), ValueError, "bhr_set_spin", "spin 0", "kerr disk v2 source")
    refused(lambda: r.set_kerr_anti_alias(True, 1.0), ValueError, "bhr_set_kerr_anti_alias", "kerr disk v2 source", "mip chain")
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True, kerr_observer=(0.0, 0.0, 0.0)), ValueError, "bhr_render_kerr_view", "kerr disk v2 source", "disk texture")
    refused(lambda: r.build_kerr_ray_map(view, 90.0), ValueError, "bhr_kerr_raymap_build", "kerr disk v2 source", "disk texture")
    cam = r.camera_uniforms(view, 90.0)
    cams = (_lib.Camera * 2)(cam, cam)
    refused(lambda: _lib.check(r._lib.bhr_kerr_raymap_render_shutter(r._ctx, cams, 2, _lib.SKIP_BLOOM)), ValueError, "bhr_kerr_raymap_render_shutter",
            "kerr disk v2 source", "disk texture")
    # what every Kerr frame refuses stays refused: the persistent schedule, adaptive supersampling
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True, compaction=True), ValueError, "spin", "persistent")
    r.set_supersample(2, 0.1)
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True), ValueError, "spin", "adaptive")
    r.set_supersample(1)
    # the volume and the exact redshift, in either order of calls
    r.set_redshift("exact")                                # the surface takes it
    refused(lambda: r.use_kerr_disk_v2(P, volume=True), ValueError, "bhr_set_kerr_disk_source", "volume", "exact redshift")
    assert r.kerr_disk_model == "v2"
    r.set_redshift("model")
    r.use_kerr_disk_v2(P, volume=True)
    refused(lambda: r.set_redshift("exact"), ValueError, "bhr_set_redshift", "exact redshift", "volume")
    r.render_async(view, 90.0, skip_bloom=True)            # the context is as it was: a volume frame still renders
    assert r.read_layer(_lib.LAYER_DISK).max() > 0
    r.use_kerr_disk_v2(None)
    r.set_spin(0.0)                                        # ... and without the source the spin goes
    r.close()

    # setting the source while the Kerr anti-aliasing is on, or a Kerr ray map is built
    r = _renderer(case)
    r.set_kerr_anti_alias(True, 1.0)
    refused(lambda: r.use_kerr_disk_v2(P), ValueError, "bhr_set_kerr_disk_source", "kerr anti-aliasing", "mip chain")
    r.set_kerr_anti_alias(False)
    r.build_kerr_ray_map(view, 90.0)
    refused(lambda: r.use_kerr_disk_v2(P, volume=True), ValueError, "bhr_set_kerr_disk_source", "kerr ray map is built", "disk texture")
    _lib.check(r._lib.bhr_kerr_raymap_free(r._ctx))
    r.use_kerr_disk_v2(P)
    r.close()

    # use_disk_v2 with set_spin is refused exactly as today
    r = _renderer(case, kerr=False)
    r.use_disk_v2(P)
    refused(lambda: r.set_spin(0.5), ValueError, "spin", "disk v2")
    r.close()
    r = _renderer(case)
    r.use_disk_v2(P)
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True), ValueError, "spin 0.5 with a disk v2 source (1): the kerr march shades the disk texture")
    r.close()


def test_back_to_the_texture_is_the_frame_of_a_context_that_never_left_it(hip_lib):
    case = DC.Case("surface", 0.6, KC.VIEWS[0], width=48, height=32)
    r = _renderer(case)
    never = _layers(r, case)
    counters = r.counters()
    r.close()
    r = _renderer(case)
    for volume in (False, True):
        r.use_kerr_disk_v2(DC.params(case)[0], volume=volume)
        other = _layers(r, case)
        assert not np.array_equal(other["disk"], never["disk"])
        r.use_kerr_disk_v2(None)
        back = _layers(r, case)
        for layer in ("bg", "disk", "final"):
            assert np.array_equal(back[layer], never[layer]), layer
        assert r.counters()["march_vgprs"] == counters["march_vgprs"] and r.kerr_disk_model == "texture"
    r.close()


# ---- 9: resources -----------------------------------------------------------------------------------------------------------------------
def test_resources(hip_lib):
    from bhr_amd import _lib
    case = DC.Case("surface", 0.9, KC.VIEWS[0], width=16, height=8)
    r = _renderer(case)
    texture = r.kerr_resources()
    for redshift in ("model", "exact"):
        for ss in (False, True):
            res = r.kerr_disk_resources(volume=False, supersampled=ss, redshift=redshift)
            print(f"surface {redshift} supersampled={ss}: {res}")
            assert res["scratch_bytes"] == 0 and res["vgprs"] > 0 and res["lds_bytes"] == texture["lds_bytes"]
    for ss in (False, True):
        res = r.kerr_disk_resources(volume=True, supersampled=ss)
        print(f"volume supersampled={ss}: {res}")
        assert res["vgprs"] > 0 and res["lds_bytes"] == texture["lds_bytes"]
    with pytest.raises(ValueError, match="volume"):
        r.kerr_disk_resources(volume=True, redshift="exact")
    import ctypes as C
    out = (C.c_int32 * 3)()
    assert r._lib.bhr_kerr_disk_resources(0, 0, 0, out) == _lib.BHR_ERR_INVALID
    # the counters name the kernel that marches the frame
    assert r.counters()["march_vgprs"] == texture["vgprs"]
    r.use_kerr_disk_v2(DC.params(case)[0])
    assert r.counters()["march_vgprs"] == r.kerr_disk_resources()["vgprs"]
    r.set_redshift("exact")
    assert r.counters()["march_vgprs"] == r.kerr_disk_resources(redshift="exact")["vgprs"]
    r.set_redshift("model")
    r.use_kerr_disk_v2(DC.params(case)[0], volume=True)
    assert r.counters()["march_vgprs"] == r.kerr_disk_resources(volume=True)["vgprs"]
    r.use_kerr_disk_v2(None)
    assert r.counters()["march_vgprs"] == texture["vgprs"]
    r.close()
