"""The spinning (Kerr) hole on the device (bhr_set_spin; csrc/ray_kerr.h) against its CPU reference tests/kerr_ref.py in
binary64, against the context's own strict Schwarzschild frame at spin 0, against the analytic shadow edges, under
supersampling, and its refusals, resources and step count.

Bars.  The device computes in f32 with v_rcp / v_rsq seeds and FMA contraction, so it is allowed twice the distance the
float32 run of kerr_ref keeps from its float64 run on the same case and layer (per-channel RMSE), and never less than the
project's 1e-4 bar.  Pixels whose fate (captured or not) or number of disk crossings differs from the float64
run sit on a discontinuity of the picture: they are counted separately, at most 0.5 % of a frame, and left out of the RMSE.
The device's fates and crossing counts are read from a probe frame: a white sky and a disk of constant opacity 1/2 per
crossing make BG = 2^-crossings for a ray that reaches the sky and 0 for any other."""
import functools

import numpy as np
import pytest

import kerr_cases as KC
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


def _fates(probe):
    """(reached the sky, crossings of such a ray or -1, a captured ray crossed the disk) of a probe frame."""
    bg = probe["bg"][..., 0].astype(np.float64)
    sky = bg > 0
    n = np.where(sky, np.rint(-np.log2(np.where(sky, bg, 1.0))), -1).astype(np.int64)
    return sky, n, probe["disk"].max(axis=2) > 0


@functools.lru_cache(maxsize=None)
def _device(A, view, force=False, spin=True, width=KC.W, height=KC.H, supersample=1):
    """Layers, counters and probe read-out of one device frame; spin=False: a context that never called set_spin."""
    from bhr_amd import HipRenderer
    out = {}
    for name, (sky, tex) in (("frame", KC.scene()), ("probe", _probe_scene())):
        r = HipRenderer(width, height, sky, tex, math="strict", supersample=supersample, **KW)
        if spin:
            r.set_spin(A, force_kerr=force)
        out[name] = _layers(r, view)
        if name == "frame":
            out["counters"] = r.counters()
            out["resources"] = r.kerr_resources()
        r.close()
    return out


def _same_as_reference(dev, ref):
    """Pixels whose fate and crossing count on the device are the float64 reference's."""
    sky, n, dark_hit = _fates(dev["probe"])
    ref_sky = ref["fate"] == 1
    same = sky == ref_sky
    same &= np.where(sky & ref_sky, n == ref["n_hits"], True)
    same &= np.where(~sky & ~ref_sky, dark_hit == (ref["n_hits"] > 0), True)
    return same


@pytest.mark.parametrize("case", KC.CASES, ids=lambda c: f"A{c[0]}-pov{c[1][0]:g}_{c[1][1]:g}")
def test_device_against_kerr_ref_float64(case, hip_lib):
    A, view = case
    r64, r32 = KC.reference(case, np.float64), KC.reference(case, np.float32)
    d32 = KC.distance(r32, r64, (r32["fate"] == r64["fate"]) & (r32["n_hits"] == r64["n_hits"]))
    dev = _device(A, view, force=(A == 0.0))
    same = _same_as_reference(dev, r64)
    got = KC.distance(dev["frame"], r64, same)
    share = float((~same).mean())
    print(f"{case}: fate / crossing count differs on {share:.3%}; device vs f64 {got}; float32 reference vs f64 {d32}")
    assert dev["frame"]["disk"].max() > 0 and dev["frame"]["bg"].max() > 0
    assert share <= FATE_SHARE
    for layer in ("bg", "disk", "final"):
        bar = max(2.0 * d32[layer], BAR_FLOOR)
        assert got[layer] <= bar, f"{layer}: RMSE {got[layer]:.3g} over the bar {bar:.3g}"


@pytest.mark.parametrize("view", KC.VIEWS, ids=lambda v: f"pov{v[0]:g}_{v[1]:g}")
def test_forced_kerr_at_spin_zero_is_the_strict_frame(view, oracle, hip_lib):
    """The Kerr kernel at A = 0 against the context's own strict Schwarzschild frame, within twice what kerr_ref (f64, A = 0)
    keeps from the oracle's strict frame; and spin 0 without the force is, byte for byte, a context that never set a spin."""
    sky, tex = KC.scene()
    o = oracle.OracleRenderer(KC.W, KC.H, sky, tex, **KW)
    _, img, disk, _ = o.render(list(view), KC.FOV, skip_differentials=True, skip_bloom=True, parts=True)
    ora = dict(bg=img.transpose(1, 0, 2), disk=disk.transpose(1, 0, 2))
    ora["final"] = np.clip(ora["bg"] + ora["disk"], 0, 1)
    r64 = KC.reference((0.0, view), np.float64)
    strict = _device(0.0, view, spin=False)
    kerr = _device(0.0, view, force=True)
    # fates and crossings: the oracle's from its own layers is not needed -- the device's strict frame carries the probe
    s_sky, s_n, s_dark = _fates(strict["probe"])
    k_sky, k_n, k_dark = _fates(kerr["probe"])
    same = (s_sky == k_sky) & (s_n == k_n) & (s_dark == k_dark)
    same_ref = _same_as_reference(strict, r64)
    d_ref = KC.distance(ora, r64, same_ref)
    got = KC.distance(kerr["frame"], strict["frame"], same)
    share = float((~same).mean())
    print(f"{view}: forced Kerr vs strict: fate / crossing count differs on {share:.3%}; distance {got}; kerr_ref f64 vs oracle strict {d_ref}")
    assert share <= FATE_SHARE and float((~same_ref).mean()) <= FATE_SHARE
    for layer in ("bg", "disk", "final"):
        bar = max(2.0 * d_ref[layer], BAR_FLOOR)
        assert got[layer] <= bar, f"{layer}: RMSE {got[layer]:.3g} over the bar {bar:.3g}"
    unforced = _device(0.0, view, force=False)
    for layer in ("bg", "disk", "final"):
        assert np.array_equal(unforced["frame"][layer], strict["frame"][layer]), layer
    assert unforced["counters"]["ray_steps"] == strict["counters"]["ray_steps"]


def _shadow_row(A):
    from bhr_amd import HipRenderer, _lib
    # 90 degrees ACROSS the 257 pixels: this project's fov is the vertical one (build_camera), so the 9 rows get the angle
    # whose tangent is 9 / 257 of tan(45 degrees); the pitch of L_z / E along the row is then 6 * 2 / 257 = 0.047
    W, H, pos = 257, 9, [6.0, 0.0, 0.0]
    fov = float(np.degrees(2.0 * np.arctan(H / W)))
    sky = np.ones((16, 32, 3), dtype=np.float32)
    tex = np.zeros((8, 16, 4), dtype=np.float32)
    r = HipRenderer(W, H, sky, tex, math="strict", **KW)
    r.set_spin(A)
    r.render_async(pos, fov, skip_bloom=True)
    final = r.read_layer(_lib.LAYER_FINAL)
    r.close()
    cam = K.build_camera(pos, fov, W, H, KC.R_MAX)
    d = K.pixel_rays(cam)[H // 2]
    x0 = np.broadcast_to(cam["pos"].astype(np.float64), d.shape)
    lz = K.l_z(x0, K.initial_momentum(x0, d, A * K.M))
    return final[H // 2], lz, np.abs(d[:, 2]).max()


def test_shadow_edges_on_the_device(hip_lib):
    rows = {}
    for A in (0.9, -0.9):
        row, lz, dz = _shadow_row(A)
        assert dz < 1e-6                                           # the middle row is equatorial
        assert ((row == 0) | (row > 0.999)).all()                 # the white sky or nothing
        lo, hi = sorted(K.shadow_edges(A))
        inside = (lz > lo) & (lz < hi)
        near = (np.abs(lz - lo) < 0.01) | (np.abs(lz - hi) < 0.01)
        black = (row == 0).all(axis=1)
        print(f"A={A}: edges {lo:.5f} {hi:.5f}, black pixels {int(black.sum())}, left out {int(near.sum())}, pitch {np.abs(np.diff(lz)).max():.4f}")
        assert near.sum() <= 2 and 0.04 < np.abs(np.diff(lz)).max() < 0.05
        assert np.array_equal(black[~near], inside[~near])
        rows[A] = (black, near)
    # a hole of the opposite spin is the mirror image
    free = ~(rows[0.9][1] | rows[-0.9][1][::-1])
    assert np.array_equal(rows[0.9][0][free], rows[-0.9][0][::-1][free])
    assert rows[0.9][0].sum() > 20 and not np.array_equal(rows[0.9][0], rows[0.9][0][::-1])      # a shifted shadow


def _ulp_close(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def test_supersampled_frame_is_the_box_filter_of_the_fine_frame(hip_lib):
    """A --supersample 2 Kerr frame against the box filter of the 192 x 128 Kerr frame of the same configuration (a context has
    one frame size, so the fine frame comes from a second context), within 1 ulp per value; the same rays, so the same steps."""
    A, view = 0.6, KC.VIEWS[0]
    ss = _device(A, view, supersample=2)
    fine = _device(A, view, width=2 * KC.W, height=2 * KC.H)
    for layer in ("bg", "disk"):
        want = box_resolve(fine["frame"][layer], 2)
        bad = int((~_ulp_close(ss["frame"][layer], want)).any(axis=2).sum())
        assert bad == 0, f"{layer}: {bad} pixels more than 1 ulp from the box filter of the 192 x 128 frame"
    assert ss["counters"]["rays"] == 4 * KC.W * KC.H
    assert ss["counters"]["ray_steps"] == fine["counters"]["ray_steps"]
    assert ss["frame"]["disk"].max() > 0


@pytest.mark.parametrize("math", ["hybrid", "fast"])
def test_math_mode_does_not_select_the_march_and_the_bloom_follows_it(math, hip_lib):
    """The CLI's default context is math hybrid with the bloom on: the Kerr kernel then also stores the split-f16 post-pass's
    operands.  BG, DISK and the step count are the strict-mode Kerr frame's, bit for bit; FINAL is the combine of the layers."""
    from bhr_amd import HipRenderer, _lib
    A, view = 0.6, KC.VIEWS[0]
    want = _device(A, view)
    sky, tex = KC.scene()
    r = HipRenderer(KC.W, KC.H, sky, tex, math=math, **KW)
    r.set_spin(A)
    r.render_async(list(view), KC.FOV)
    got = {k: r.read_layer(v) for k, v in (("bg", _lib.LAYER_BG), ("disk", _lib.LAYER_DISK), ("blur", _lib.LAYER_BLUR), ("final", _lib.LAYER_FINAL))}
    c = r.counters()
    r.close()
    for layer in ("bg", "disk"):
        assert np.array_equal(got[layer], want["frame"][layer]), layer
    assert c["ray_steps"] == want["counters"]["ray_steps"] and c["march_vgprs"] == want["resources"]["vgprs"]
    assert np.isfinite(got["final"]).all() and (got["blur"] >= 0).all() and got["blur"].max() > 0
    combine = np.clip((got["bg"] + got["disk"]) + got["blur"], 0, 1)
    assert np.abs(got["final"] - combine).max() <= 1e-6


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
    for bad in (0.999, -1.5, float("nan")):
        with pytest.raises(ValueError):
            r.set_spin(bad)
        refused(lambda: _lib.check(r._lib.bhr_set_spin(r._ctx, bad, 0)), "0.998")
    r.close()
    r = renderer(disk_tilt=10.0)
    refused(lambda: r.set_spin(0.5), "spin", "tilt")
    refused(lambda: r.set_spin(0.0, force_kerr=True), "spin", "tilt")
    r.set_spin(0.0)                                   # no spin, no refusal
    r.close()
    r = renderer(anti_alias="lod_radius")
    refused(lambda: r.set_spin(0.5), "spin", "anti_alias")
    r.close()
    r = renderer()
    r.use_disk_v2(DiskV2Params())
    refused(lambda: r.set_spin(0.5), "spin", "disk v2")
    r.close()
    r = renderer()                                    # ... and the other way round: the source after the spin, met by the render
    r.set_spin(0.5)
    r.use_disk_v2(DiskV2Params())
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True), "spin", "disk v2")
    r.close()
    r = renderer(supersample=2, supersample_threshold=0.1)
    refused(lambda: r.set_spin(0.5), "spin", "adaptive")
    r.close()
    r = renderer()
    r.set_spin(0.5)
    r.set_supersample(2, 0.1)
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True), "spin", "adaptive")
    r.set_supersample(1)
    refused(lambda: r.render_async(view, 90.0, skip_bloom=True, compaction=True), "spin", "persistent")
    refused(lambda: r.build_ray_map(view, 90.0), "spin", "ray map")
    refused(lambda: r.render_from_ray_map_async(), "spin", "ray map")
    refused(lambda: r.render_shutter_async([view, view], 90.0, [0.0, 0.1], skip_bloom=True), "spin", "shutter")
    cam = r.camera_uniforms(view, 90.0)
    import ctypes as C
    ctxs = (C.c_void_p * 1)(r._ctx)
    refused(lambda: _lib.check(r._lib.bhr_group_render(ctxs, 1, C.byref(cam), _lib.SKIP_BLOOM, None)), "spin", "group")
    refused(lambda: _lib.check(r._lib.bhr_tile_render(r._ctx, C.byref(cam), _lib.SKIP_BLOOM)), "spin", "tile")
    r.render_async(view, 90.0, skip_bloom=True)       # the context is as it was: a Kerr frame still renders
    assert r.read_layer(_lib.LAYER_BG).max() > 0
    r.close()
    r = renderer(rows=(0, 8))
    refused(lambda: r.set_spin(0.5), "spin", "row-block")
    r.close()


def test_resources_and_step_count(hip_lib):
    total, total_ref = 0, 0
    for case in KC.CASES:
        A, view = case
        dev = _device(A, view, force=(A == 0.0))
        res = dev["resources"]
        assert res["scratch_bytes"] == 0 and res["vgprs"] > 0 and res["lds_bytes"] > 0
        assert dev["counters"]["march_vgprs"] == res["vgprs"] and dev["counters"]["march_lds_bytes"] == res["lds_bytes"]
        steps, want = int(dev["counters"]["ray_steps"]), int(KC.reference(case, np.float32)["steps"].sum())
        print(f"{case}: ray steps {steps}, float32 reference {want}, off by {abs(steps - want) / want:.2e}; {res}")
        assert abs(steps - want) <= 2e-4 * want
        total, total_ref = total + steps, total_ref + want
    assert abs(total - total_ref) <= 2e-4 * total_ref
    from bhr_amd import HipRenderer
    sky, tex = KC.scene()
    r = HipRenderer(16, 8, sky, tex, **KW)
    r.set_spin(0.9)
    info = r.kerr_info()
    twin = r.kerr_resources(supersampled=True)          # the supersampled twin must not spill either
    print(f"supersampled twin: {twin}")
    assert twin["scratch_bytes"] == 0 and twin["vgprs"] > 0 and twin["lds_bytes"] > 0
    r.close()
    want = K.kerr_info(0.9)
    assert set(info) == {"a", "r_plus", "r_isco_prograde", "r_isco_retrograde", "r_photon_pro", "r_photon_retro"}
    for k in want:
        assert info[k] == pytest.approx(want[k], abs=1e-12), k
