"""The exact Kerr disk redshift on the device (bhr_set_redshift, BHR_REDSHIFT_EXACT; csrc/ray_kerr.h: kerr_g_exact) against its
CPU reference tests/kerr_redshift_ref.py in binary64, against the model frames of the same context (the march is shared: BG and
the step count do not move), under supersampling, and its refusals and resources.

Bars: those of tests/test_gpu_kerr.py.  The device is allowed twice the distance the float32 run of the reference keeps from
its float64 run on the same case and layer (per-channel RMSE), never less than 1e-4; pixels whose fate or number of disk
crossings differs from the float64 run are counted separately, at most 0.5 % of a frame, and left out of the RMSE.  Fates and
crossing counts are read from a probe frame (a white sky, a disk of opacity 1/2 per crossing)."""
import functools

import numpy as np
import pytest

import kerr_cases as KC
import kerr_redshift_ref as R
import kerr_ref as K
from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

KW = dict(step_size=KC.STEP, r_max=KC.R_MAX, r_disk_inner=KC.R_INNER, r_disk_outer=KC.R_OUTER, disk_tilt=0.0, anti_alias="disabled")
BAR_FLOOR = 1e-4
FATE_SHARE = 0.005
PROBE_ALPHA = float(1.0 - 0.5 ** (1.0 / 6.0))        # disk_alpha = 1 - (1 - alpha)^6 = 1/2


def _probe_scene():
    sky = np.ones((16, 32, 3), dtype=np.float32)
    tex = np.ones((8, 16, 4), dtype=np.float32)
    tex[..., 3] = PROBE_ALPHA
    return sky, tex


def _layers(r, view, fov=KC.FOV):
    from bhr_amd import _lib
    r.render_async(list(view), fov, skip_bloom=True)
    return dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), final=r.read_layer(_lib.LAYER_FINAL))


@functools.lru_cache(maxsize=None)
def _reference(case, dtype, width=KC.W, height=KC.H):
    """kerr_redshift_ref's frame of a case (read-only: shared between tests)."""
    A, view = case
    sky, tex = KC.scene()
    cam = K.build_camera(list(view), KC.FOV, width, height, KC.R_MAX)
    out = R.render(cam, A, sky, tex, h_base=KC.STEP, r_inner=KC.R_INNER, r_outer=KC.R_OUTER, dtype=dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _device(A, view, redshift="exact", width=KC.W, height=KC.H, supersample=1):
    """Layers, counters and probe read-out of one device frame; redshift None: a context that never called set_redshift (a spin
    of 0 is then the forced Kerr march, as in tests/test_gpu_kerr.py)."""
    from bhr_amd import HipRenderer
    out = {}
    for name, (sky, tex) in (("frame", KC.scene()), ("probe", _probe_scene())):
        r = HipRenderer(width, height, sky, tex, math="strict", supersample=supersample, **KW)
        r.set_spin(A, force_kerr=(A == 0.0))
        if redshift is not None:
            r.set_redshift(redshift)
            assert r.redshift == redshift
        out[name] = _layers(r, view)
        if name == "frame":
            out["counters"] = r.counters()
        r.close()
    return out


def _same_as_reference(dev, ref):
    """Pixels whose fate and crossing count on the device are the float64 reference's."""
    bg = dev["probe"]["bg"][..., 0].astype(np.float64)
    sky = bg > 0
    n = np.where(sky, np.rint(-np.log2(np.where(sky, bg, 1.0))), -1).astype(np.int64)
    dark_hit = dev["probe"]["disk"].max(axis=2) > 0
    ref_sky = ref["fate"] == 1
    same = sky == ref_sky
    same &= np.where(sky & ref_sky, n == ref["n_hits"], True)
    same &= np.where(~sky & ~ref_sky, dark_hit == (ref["n_hits"] > 0), True)
    return same


@pytest.mark.parametrize("case", KC.CASES, ids=lambda c: f"A{c[0]}-pov{c[1][0]:g}_{c[1][1]:g}")
def test_device_exact_against_the_reference_float64(case, hip_lib):
    A, view = case
    r64, r32 = _reference(case, np.float64), _reference(case, np.float32)
    d32 = KC.distance(r32, r64, (r32["fate"] == r64["fate"]) & (r32["n_hits"] == r64["n_hits"]))
    dev = _device(A, view)
    same = _same_as_reference(dev, r64)
    got = KC.distance(dev["frame"], r64, same)
    share = float((~same).mean())
    hits = np.sqrt((r64["first_hit"] ** 2).sum(-1) - (A * K.M) ** 2)
    inside = int((hits < R.isco_orbit(A)[0]).sum())
    print(f"{case}: fate / crossing count differs on {share:.3%}; device vs f64 {got}; float32 reference vs f64 {d32}; "
          f"first crossings inside / outside the ISCO {inside} / {int(np.isfinite(hits).sum()) - inside}")
    assert dev["frame"]["disk"].max() > 0 and dev["frame"]["bg"].max() > 0
    assert share <= FATE_SHARE
    for layer in ("bg", "disk", "final"):
        bar = max(2.0 * d32[layer], BAR_FLOOR)
        assert got[layer] <= bar, f"{layer}: RMSE {got[layer]:.3g} over the bar {bar:.3g}"


def test_both_branches_are_covered():
    """The cases reach both sides of the ISCO (read from the reference's first crossings; no device)."""
    inside = outside = 0
    for case in KC.CASES:
        A = case[0]
        first = _reference(case, np.float64)["first_hit"]
        r = np.sqrt((first ** 2).sum(-1) - (A * K.M) ** 2)
        inside += int((r < R.isco_orbit(A)[0]).sum())
        outside += int((r >= R.isco_orbit(A)[0]).sum())
    assert inside > 500 and outside > 500


def test_exact_changes_the_shading_only_and_model_restores_the_frame(hip_lib):
    from bhr_amd import HipRenderer
    sky, tex = KC.scene()
    for A in (0.6, -0.9):
        view = KC.VIEWS[0]
        never = _device(A, view, redshift=None)
        r = HipRenderer(KC.W, KC.H, sky, tex, math="strict", **KW)
        r.set_spin(A)
        assert r.redshift == "model"
        model, c_model = _layers(r, view), r.counters()
        r.set_redshift("exact")
        exact, c_exact = _layers(r, view), r.counters()
        r.set_redshift("model")
        back, c_back = _layers(r, view), r.counters()
        r.close()
        assert np.array_equal(model["bg"], exact["bg"]) and c_model["ray_steps"] == c_exact["ray_steps"]
        diff = np.abs(model["disk"] - exact["disk"])
        print(f"A={A}: DISK layer model vs exact: mean |difference| {diff.mean():.3g}, largest {diff.max():.3g}, {float((diff > 0).any(axis=2).mean()):.1%} of the pixels")
        assert diff.max() > 1e-2
        # the exact frame is the one a context made for it renders
        want = _device(A, view)
        for layer in ("bg", "disk", "final"):
            assert np.array_equal(exact[layer], want["frame"][layer]), layer
            assert np.array_equal(model[layer], never["frame"][layer]), layer
            assert np.array_equal(back[layer], never["frame"][layer]), layer
        assert c_back["ray_steps"] == never["counters"]["ray_steps"]
        assert c_back["march_vgprs"] == never["counters"]["march_vgprs"]
    # at spin 0 "exact" turns the Kerr march on itself and "model" turns it off again: the strict Schwarzschild frame is back
    view = KC.VIEWS[1]
    r = HipRenderer(KC.W, KC.H, sky, tex, math="strict", **KW)
    plain, c_plain = _layers(r, view), r.counters()
    r.set_redshift("exact")
    exact = _layers(r, view)
    assert r.spin == 0.0 and r.redshift == "exact"
    r.set_redshift("model")
    back, c_back = _layers(r, view), r.counters()
    r.close()
    want = _device(0.0, view)
    for layer in ("bg", "disk", "final"):
        assert np.array_equal(exact[layer], want["frame"][layer]), layer
        assert np.array_equal(back[layer], plain[layer]), layer
    assert c_back["ray_steps"] == c_plain["ray_steps"] and c_back["march_vgprs"] == c_plain["march_vgprs"]
    # ... and the keyword is the call
    r = HipRenderer(KC.W, KC.H, sky, tex, math="strict", redshift="exact", **KW)
    kw_frame = _layers(r, view)
    r.close()
    assert np.array_equal(kw_frame["disk"], want["frame"]["disk"])


def _ulp_close(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def test_supersampled_exact_frame_is_the_box_filter_of_the_fine_frame(hip_lib):
    A, view = -0.9, KC.VIEWS[0]
    ss = _device(A, view, supersample=2)
    fine = _device(A, view, width=2 * KC.W, height=2 * KC.H)
    for layer in ("bg", "disk"):
        want = box_resolve(fine["frame"][layer], 2)
        bad = int((~_ulp_close(ss["frame"][layer], want)).any(axis=2).sum())
        assert bad == 0, f"{layer}: {bad} pixels more than 1 ulp from the box filter of the 192 x 128 frame"
    assert ss["counters"]["rays"] == 4 * KC.W * KC.H
    assert ss["counters"]["ray_steps"] == fine["counters"]["ray_steps"]
    assert ss["frame"]["disk"].max() > 0
    assert not np.array_equal(ss["frame"]["disk"], _device(A, view, redshift=None, supersample=2)["frame"]["disk"])


def test_refusals(hip_lib):
    from bhr_amd import HipRenderer, _lib
    from bhr_amd.disk_v2 import DiskV2Params
    sky, tex = KC.scene()
    W, H, view = 32, 16, [6.0, 0.0, 0.5]

    def renderer(**kw):
        return HipRenderer(W, H, sky, tex, **dict(KW, **kw))

    def refused(fn, *words):
        with pytest.raises(ValueError) as e:
            fn()
        msg = str(e.value).lower()
        assert all(w in msg for w in words), msg

    r = renderer()
    # the C entry point: EXACT without the Kerr march, an unknown mode
    refused(lambda: _lib.check(r._lib.bhr_set_redshift(r._ctx, _lib.REDSHIFT_EXACT)), "exact", "kerr", "bhr_set_spin")
    for bad in (2, -1):
        refused(lambda: _lib.check(r._lib.bhr_set_redshift(r._ctx, bad)), "unknown mode")
    _lib.check(r._lib.bhr_set_redshift(r._ctx, _lib.REDSHIFT_MODEL))                     # the default, at any spin
    with pytest.raises(ValueError):
        r.set_redshift("doppler")
    with pytest.raises(ValueError):
        r.kerr_resources(redshift="doppler")
    import ctypes as C
    out = (C.c_int32 * 3)()
    refused(lambda: _lib.check(r._lib.bhr_kerr_redshift_resources(7, 0, out)), "unknown mode")
    # dropping the spin while EXACT is set
    r.set_spin(0.5)
    r.set_redshift("exact")
    refused(lambda: r.set_spin(0.0), "spin 0", "exact", "bhr_set_redshift")
    refused(lambda: _lib.check(r._lib.bhr_set_spin(r._ctx, 0.0, 0)), "exact")
    assert r.spin == 0.5 and r.redshift == "exact"
    r.set_spin(0.0, force_kerr=True)                                                       # the Kerr march stays on: fine
    r.set_spin(-0.3)
    # what a spin refuses at render time is refused under exact
    r.use_disk_v2(DiskV2Params())
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True), "spin", "disk v2")
    r.close()
    r = renderer()
    r.set_redshift("exact")                           # spin 0: the forced Kerr march
    r.set_supersample(2, 0.1)
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True), "spin", "adaptive")
    r.set_supersample(1)
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True, compaction=True), "spin", "persistent")
    refused(lambda: r.build_ray_map(view, 90.0), "spin", "ray map")
    refused(lambda: r.render_from_ray_map_async(), "spin", "ray map")
    refused(lambda: r.render_shutter_async([view, view], 90.0, [0.0, 0.1], skip_bloom=True), "spin", "shutter")
    cam = r.camera_uniforms(view, 90.0)
    ctxs = (C.c_void_p * 1)(r._ctx)
    refused(lambda: _lib.check(r._lib.bhr_group_render(ctxs, 1, C.byref(cam), _lib.SKIP_BLOOM, None)), "spin", "group")
    refused(lambda: _lib.check(r._lib.bhr_tile_render(r._ctx, C.byref(cam), _lib.SKIP_BLOOM)), "spin", "tile")
    r.render_async(view, 90.0, skip_bloom=True)       # the context is as it was: an exact frame still renders
    assert r.read_layer(_lib.LAYER_DISK).max() > 0
    r.close()
    # ... and each state a spin refuses, met by set_redshift("exact") at spin 0; the context stays a Schwarzschild one
    for kw, words in ((dict(disk_tilt=10.0), ("spin", "tilt")), (dict(anti_alias="lod_radius"), ("spin", "anti_alias")),
                      (dict(supersample=2, supersample_threshold=0.1), ("spin", "adaptive")), (dict(rows=(0, 8)), ("spin", "row-block"))):
        r = renderer(**kw)
        refused(lambda: r.set_redshift("exact"), *words)
        assert r.redshift == "model" and r.spin == 0.0
        refused(lambda: HipRenderer(W, H, sky, tex, redshift="exact", **dict(KW, **kw)), *words)
        r.close()
    r = renderer()
    r.use_disk_v2(DiskV2Params())
    refused(lambda: r.set_redshift("exact"), "spin", "disk v2")
    r.close()


def test_resources(hip_lib):
    from bhr_amd import HipRenderer
    sky, tex = KC.scene()
    r = HipRenderer(16, 8, sky, tex, **KW)
    model = r.kerr_resources()
    assert r.kerr_resources(redshift="model") == model
    for ss in (False, True):
        res = r.kerr_resources(supersampled=ss, redshift="exact")
        print(f"exact, supersampled {ss}: {res}; model: {r.kerr_resources(supersampled=ss)}")
        assert 0 < res["vgprs"] <= 128 and res["scratch_bytes"] == 0 and res["lds_bytes"] == model["lds_bytes"]
    r.set_spin(0.9)
    r.set_redshift("exact")
    c = r.counters()
    res = r.kerr_resources(redshift="exact")
    assert c["march_vgprs"] == res["vgprs"] and c["march_lds_bytes"] == res["lds_bytes"]
    r.close()
