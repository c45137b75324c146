"""The Kerr anti-aliasing on the device (bhr_set_kerr_anti_alias; csrc/ray_kerr.h "Ray differentials") against its CPU reference
tests/kerr_aa_ref.py in binary64, against the frame without the switch, under other settings, under supersampling, against the
context's own strict anti-aliased frame at spin 0, and its refusals and resources.

Bars are tests/test_gpu_kerr.py's: twice the distance the float32 run of the reference keeps from its float64 run on the same
case and layer (per-channel RMSE), never less than 1e-4; the pixels whose fate or crossing count differs from the float64 run
are at most 0.5 % of a frame and left out, and so are the pixels with a crossing whose lod lies within kerr_aa_cases.DELTA of a
jump of the mip level (at most 5 % of the pixels that have a crossing; tests/test_kerr_aa_ref.py checks that of the inputs).
Fates and crossing counts of the device come from a probe frame: a white sky and a disk of constant opacity 1/2 per crossing."""
import functools

import numpy as np
import pytest

import kerr_aa_cases as AC
import kerr_cases as KC
from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

KW = dict(step_size=KC.STEP, r_max=KC.R_MAX, r_disk_outer=KC.R_OUTER, disk_tilt=0.0, anti_alias="disabled")
BAR_FLOOR = 1e-4
FATE_SHARE = 0.005
PROBE_ALPHA = float(1.0 - 0.5 ** (1.0 / 6.0))        # disk_alpha = 1 - (1 - alpha)^6 = 1/2


def _scenes(name):
    sky, tex = KC.scene()
    if name == "probe":
        sky, tex = np.ones((16, 32, 3), dtype=np.float32), np.ones((8, 16, 4), dtype=np.float32)
        tex[..., 3] = PROBE_ALPHA
    elif name == "clear":                            # the frame's disk with opacity 0 at every level: BG is the sky of every ray
        tex = tex.copy()
        tex[..., 3] = 0.0
    return sky, tex


@functools.lru_cache(maxsize=None)
def _device(A, view, aa=1.0, force=False, width=KC.W, height=KC.H, supersample=1, redshift="model", fov=KC.FOV, r_inner=KC.R_INNER,
            scenes=("frame", "probe")):
    """Layers of one device frame per scene, the frame's counters and the kernel's resources; aa: the LOD strength, None: off."""
    from bhr_amd import HipRenderer, _lib
    out = {}
    for name in scenes:
        sky, tex = _scenes(name)
        r = HipRenderer(width, height, sky, tex, math="strict", supersample=supersample, r_disk_inner=r_inner, **KW)
        r.set_spin(A, force_kerr=force)
        if redshift != "model":
            r.set_redshift(redshift)
        if aa is not None:
            r.set_kerr_anti_alias(True, aa)
        r.render_async(list(view), fov, skip_bloom=True)
        out[name] = dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), final=r.read_layer(_lib.LAYER_FINAL))
        if name == scenes[0]:
            out["counters"] = r.counters()
            out["resources"] = (r.kerr_anti_alias_resources(supersample > 1, redshift) if aa is not None
                                else r.kerr_resources(supersample > 1, redshift))
        r.close()
    return out


def _fates(probe):
    """(reached the sky, crossings of such a ray or -1, a captured ray crossed the disk) of a probe frame."""
    bg = probe["bg"][..., 0].astype(np.float64)
    sky = bg > 0
    n = np.where(sky, np.rint(-np.log2(np.where(sky, bg, 1.0))), -1).astype(np.int64)
    return sky, n, probe["disk"].max(axis=2) > 0


def _same_as_reference(dev, ref):
    sky, n, dark_hit = _fates(dev["probe"])
    ref_sky = ref["fate"] == 1
    same = sky == ref_sky
    same &= np.where(sky & ref_sky, n == ref["n_hits"], True)
    same &= np.where(~sky & ~ref_sky, dark_hit == (ref["n_hits"] > 0), True)
    return same


def _check_against_reference(label, dev, r64, r32):
    away = AC.away_from_jumps(r64)
    d32 = KC.distance(r32, r64, AC.same_fate(r32, r64) & away)
    same = _same_as_reference(dev, r64)
    got = KC.distance(dev["frame"], r64, same & away)
    share, crossing = float((~same).mean()), r64["n_hits"] > 0
    jump = float((~away).sum() / max(int(crossing.sum()), 1))
    print(f"{label}: fate / crossing count differs on {share:.3%}; near a jump {jump:.3%} of the pixels with a crossing; "
          f"device vs f64 {got}; float32 reference vs f64 {d32}")
    assert dev["frame"]["bg"].max() > 0
    assert share <= FATE_SHARE
    assert jump <= AC.JUMP_SHARE
    for layer in ("bg", "disk", "final"):
        bar = max(2.0 * d32[layer], BAR_FLOOR)
        assert got[layer] <= bar, f"{layer}: RMSE {got[layer]:.3g} over the bar {bar:.3g}"


@pytest.mark.parametrize("case", KC.CASES, ids=lambda c: f"A{c[0]}-pov{c[1][0]:g}_{c[1][1]:g}")
def test_device_against_kerr_aa_ref_float64(case, hip_lib):
    A, view = case
    dev = _device(A, view, force=(A == 0.0))
    assert dev["frame"]["disk"].max() > 0
    _check_against_reference(str(case), dev, AC.reference(case, np.float64), AC.reference(case, np.float32))


def test_strength_zero_is_the_frame_without_the_switch(hip_lib):
    """lod = 0 at every crossing: level 0, whose sampler is kerr_sample_disk bit for bit.  BG, DISK and the step count."""
    A, view = 0.6, KC.VIEWS[0]
    off, zero = _device(A, view, aa=None), _device(A, view, aa=0.0)
    for layer in ("bg", "disk"):
        assert np.array_equal(off["frame"][layer], zero["frame"][layer]), layer
    assert off["counters"]["ray_steps"] == zero["counters"]["ray_steps"]
    assert zero["counters"]["march_vgprs"] == zero["resources"]["vgprs"] != off["resources"]["vgprs"]


@pytest.mark.parametrize("case", [(0.6, KC.VIEWS[0]), (0.998, KC.VIEWS[1])], ids=lambda c: f"A{c[0]}-pov{c[1][0]:g}_{c[1][1]:g}")
def test_the_tangents_do_not_touch_the_primal(case, hip_lib):
    """At any strength the rays are the rays without the switch: equal step counts, and BG byte-identical wherever it does not
    depend on the disk's opacity.  BG is the sky times (1 - alpha) of the crossings and alpha is sampled at the crossing's mip
    level, so on the frame's own scene that is every pixel without a shaded crossing; on the same scene with a disk of opacity 0
    at every level it is EVERY pixel -- the escape direction of every ray, bit for bit, those that crossed the disk included."""
    A, view = case
    scenes = ("frame", "probe", "clear")
    off, on = _device(A, view, aa=None, scenes=scenes), _device(A, view, aa=1.5, scenes=scenes)
    assert off["counters"]["ray_steps"] == on["counters"]["ray_steps"]
    sky, n, dark_hit = _fates(off["probe"])
    crossed = (sky & (n > 0)) | dark_hit
    assert crossed.mean() > 0.3 and (sky & (n > 0)).mean() > 0.2
    assert all(np.array_equal(a, b) for a, b in zip(_fates(off["probe"]), _fates(on["probe"])))      # the same fates and counts
    assert np.array_equal(off["frame"]["bg"][~crossed], on["frame"]["bg"][~crossed])
    assert np.array_equal(off["frame"]["disk"][~crossed], on["frame"]["disk"][~crossed])
    assert not np.array_equal(off["frame"]["disk"], on["frame"]["disk"])
    assert np.array_equal(off["clear"]["bg"], on["clear"]["bg"]) and on["clear"]["bg"][sky & (n > 0)].min() > 0


OTHER = {
    "strength-1.5": dict(aa=1.5),
    "exact": dict(redshift="exact"),
    "crossings": dict(fov=KC.CROSSINGS[0].fov, r_inner=KC.CROSSINGS[0].r_inner),       # three and more: the in-loop flush moves nine words
    "61x43": dict(width=61, height=43), "33x9": dict(width=33, height=9), "5x3": dict(width=5, height=3),
}


@pytest.mark.parametrize("name", list(OTHER))
def test_other_settings(name, hip_lib):
    kw = OTHER[name]
    A, view = (KC.CROSSINGS[0].A, KC.CROSSINGS[0].view) if name == "crossings" else (0.9, KC.VIEWS[1]) if "x" in name else (0.6, KC.VIEWS[0])
    dev = _device(A, view, **kw)
    ref_kw = dict(strength=kw.get("aa", 1.0), redshift=kw.get("redshift", "model"), width=kw.get("width", KC.W), height=kw.get("height", KC.H),
                  fov=kw.get("fov", KC.FOV), r_inner=kw.get("r_inner", KC.R_INNER))
    r64, r32 = AC.reference((A, view), np.float64, **ref_kw), AC.reference((A, view), np.float32, **ref_kw)
    if name == "crossings":
        assert (r64["n_hits"] >= 3).sum() > 20
    _check_against_reference(name, dev, r64, r32)


def _ulp_close(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def test_supersampled_frame_is_the_box_filter_of_the_fine_frame(hip_lib):
    """supersample=2 with the switch on against the box filter of the 192 x 128 anti-aliased frame (the direction differentials of
    a supersampled frame are the fine frame's), within 1 ulp per value; the same rays, so the same steps."""
    A, view = 0.6, KC.VIEWS[0]
    ss = _device(A, view, supersample=2, scenes=("frame",))
    fine = _device(A, view, width=2 * KC.W, height=2 * KC.H, scenes=("frame",))
    for layer in ("bg", "disk"):
        want = box_resolve(fine["frame"][layer], 2)
        bad = int((~_ulp_close(ss["frame"][layer], want)).any(axis=2).sum())
        assert bad == 0, f"{layer}: {bad} pixels more than 1 ulp from the box filter of the 192 x 128 frame"
    assert ss["counters"]["rays"] == 4 * KC.W * KC.H
    assert ss["counters"]["ray_steps"] == fine["counters"]["ray_steps"]
    assert ss["frame"]["disk"].max() > 0


@pytest.mark.parametrize("view", KC.VIEWS, ids=lambda v: f"pov{v[0]:g}_{v[1]:g}")
def test_forced_spin_zero_against_the_strict_anti_aliased_frame(view, hip_lib):
    """The anti-aliased Kerr kernel at A = 0 against the context's own strict Schwarzschild frame with anti_alias = lod_radius,
    within twice what kerr_aa_ref (f64, A = 0) keeps from the oracle's strict anti-aliased frame (kerr_aa_cases.ORACLE_DISTANCE,
    which says why the two models differ), over the pixels of equal fate and crossing count that are not near a jump."""
    from bhr_amd import HipRenderer, _lib
    strict = {}
    for name in ("frame", "probe"):
        sky, tex = _scenes(name)
        r = HipRenderer(KC.W, KC.H, sky, tex, math="strict", r_disk_inner=KC.R_INNER, **dict(KW, anti_alias="lod_radius", aa_strength=1.0))
        r.render_async(list(view), KC.FOV, skip_bloom=True)
        strict[name] = dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), final=r.read_layer(_lib.LAYER_FINAL))
        r.close()
    kerr = _device(0.0, view, force=True)
    s_sky, s_n, s_dark = _fates(strict["probe"])
    k_sky, k_n, k_dark = _fates(kerr["probe"])
    same = (s_sky == k_sky) & (s_n == k_n) & (s_dark == k_dark)
    got = KC.distance(kerr["frame"], strict["frame"], same & AC.away_from_jumps(AC.reference((0.0, view), np.float64)))
    share = float((~same).mean())
    print(f"{view}: forced anti-aliased Kerr vs strict anti-aliased: fate / crossing count differs on {share:.3%}; distance {got}; "
          f"recorded kerr_aa_ref f64 vs oracle {AC.ORACLE_DISTANCE[view]}")
    assert share <= FATE_SHARE
    for layer in ("bg", "disk", "final"):
        assert got[layer] <= 2.0 * AC.ORACLE_DISTANCE[view][layer], f"{layer}: RMSE {got[layer]:.3g}"


def test_refusals(hip_lib):
    from bhr_amd import HipRenderer, _lib
    sky, tex = KC.scene()
    W, H, view = 32, 16, [6.0, 0.0, 0.5]

    def refused(fn, *words, error=ValueError):
        with pytest.raises(error) as e:
            fn()
        msg = str(e.value).lower()
        assert all(w in msg for w in words), msg

    r = HipRenderer(W, H, sky, tex, r_disk_inner=KC.R_INNER, **KW)
    refused(lambda: r.set_kerr_anti_alias(True), "kerr march", "bhr_set_spin", error=AssertionError)       # no spin: BHR_ERR_STATE
    r.set_kerr_anti_alias(False)                          # off without a spin: nothing to refuse
    r.set_spin(0.5)
    for bad in (-0.5, float("nan"), float("inf")):
        refused(lambda: r.set_kerr_anti_alias(True, bad), "strength")
    r.set_kerr_anti_alias(True, 1.0)
    assert r.kerr_anti_alias == 1.0
    refused(lambda: r.build_kerr_ray_map(view, 90.0), "anti-aliasing", "ray map")
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True, kerr_observer=(0.1, 0.0, 0.0)), "anti-aliasing", "kerr view")
    refused(lambda: r.set_spin(0.0), "anti-aliasing", "bhr_set_spin")
    r.render_async(view, 90.0, skip_bloom=True)           # the context is as it was: an anti-aliased Kerr frame still renders
    assert r.read_layer(_lib.LAYER_DISK).max() > 0
    r.set_kerr_anti_alias(False)
    assert r.kerr_anti_alias is None
    r.build_kerr_ray_map(view, 90.0)                      # ... and off again, the map builds and the spin can go
    r.set_spin(0.0)
    r.close()
    r = HipRenderer(W, H, sky, tex, r_disk_inner=KC.R_INNER, **dict(KW, anti_alias="lod_radius"))
    refused(lambda: r.set_spin(0.5), "spin", "anti_alias", "variational equations")          # still refused, word for word
    r.close()


def test_resources(hip_lib):
    """No private segment in any of the four kernels; registers and LDS are printed."""
    from bhr_amd import HipRenderer
    sky, tex = KC.scene()
    r = HipRenderer(16, 8, sky, tex, r_disk_inner=KC.R_INNER, **KW)
    for redshift in ("model", "exact"):
        for ss in (False, True):
            res, plain = r.kerr_anti_alias_resources(ss, redshift), r.kerr_resources(ss, redshift)
            print(f"anti-aliased Kerr march, {redshift} redshift, supersampled {ss}: {res} (without: {plain})")
            assert res["scratch_bytes"] == 0 and res["vgprs"] > plain["vgprs"] and res["lds_bytes"] == plain["lds_bytes"] > 0
    r.close()
    dev = _device(0.6, KC.VIEWS[0])
    assert dev["counters"]["march_vgprs"] == dev["resources"]["vgprs"] and dev["counters"]["march_lds_bytes"] == dev["resources"]["lds_bytes"]
