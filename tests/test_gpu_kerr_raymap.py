"""The Kerr ray map (bhr_kerr_raymap_*; include/bhr.h states the contract, csrc/march_kerr_raymap.hip has the kernels): a
spinning hole's view marched once, every frame shaded from its records.

A map frame is the marched Kerr frame of the same context bit for bit -- the shade kernel is made of the march's own device
functions in an object with the march's flags -- on whole and ragged frames, with and without pixels on the overflow list.  A
turned view (an orbit frame) shades the build view's rays turned about z, the spin axis: checked against the same rays under a
rolled scene, with two Kerr marches of symmetric views as the bar, and against kerr_ref / kerr_redshift_ref in binary64.

Scene and constants: tests/kerr_cases.py (96 x 64, fov 90, step 0.1, analytic_skybox + noisy_disk, both 512 columns wide)."""
import json
import os

import numpy as np
import pytest

import kerr_cases as KC

pytestmark = pytest.mark.gpu

KW = dict(step_size=KC.STEP, r_max=KC.R_MAX, r_disk_inner=KC.R_INNER, r_disk_outer=KC.R_OUTER, disk_tilt=0.0, anti_alias="disabled",
          disk_rotation_speed=0.1)
FATE_SHARE = 0.005                                   # tests/test_gpu_kerr.py: the cap on fate / crossing disagreement
PROBE_ALPHA = float(1.0 - 0.5 ** (1.0 / 6.0))        # disk_alpha = 1 - (1 - alpha)^6 = 1/2 (tests/test_gpu_kerr.py's probe)
# (t_offset of the map frame, frame number of the marched one: float32(frame * 0.1) is the same float)
ROLLS = ((0.0, 0), (7.3, 73), (float(np.float32(400 * 0.1)), 400))


def _scene(roll=0):
    """The scene, its sky and texture rolled by -roll columns: what the build view's rays see in place of a turn by 2 pi roll / 512."""
    sky, tex = KC.scene()
    assert sky.shape[1] == tex.shape[1] == 512
    if roll == 0:
        return sky, tex
    return np.ascontiguousarray(np.roll(sky, -roll, axis=1)), np.ascontiguousarray(np.roll(tex, -roll, axis=1))


def _mk(A, redshift="model", force=False, width=KC.W, height=KC.H, scene=None, **kw):
    from bhr_amd import HipRenderer
    sky, tex = _scene() if scene is None else scene
    r = HipRenderer(width, height, sky, tex, math="strict", **{**KW, **kw})
    if A != 0.0 or force:
        r.set_spin(A, force_kerr=force)
    if redshift == "exact":
        r.set_redshift("exact")
    return r


def _set_scene(r, roll):
    from bhr_amd import _lib
    sky, tex = _scene(roll)
    _lib.check(r._lib.bhr_set_skybox(r._ctx, _lib.fptr(sky), sky.shape[0], sky.shape[1]))
    r.update_disk_texture(tex)


def _read(r, names=("final", "bg", "disk"), u8=True):
    from bhr_amd import _lib
    ids = dict(final=_lib.LAYER_FINAL, bg=_lib.LAYER_BG, disk=_lib.LAYER_DISK)
    out = {k: r.read_layer(ids[k]) for k in names}
    if u8:
        out["u8"] = r.read_final_u8()
    return out


def _assert_equal(got, want, tag):
    for k in want:
        bad = int((got[k] != want[k]).sum())
        assert np.array_equal(got[k], want[k]) and bad == 0, f"{tag} {k}: {bad} values differ"


def _cam(k, n=512, pov=KC.VIEWS[0]):
    from bhr_amd.camera import orbit_position
    return [float(v) for v in orbit_position(list(pov), k, n)]


def _identity(r, view, fov, tag, rolls=ROLLS, swap=True):
    """Build the map of `view`, then: every roll's map frame is the marched frame, also after a scene swap; the step counts agree;
    the frame is not blank.  Returns the map's info and passes."""
    r.build_kerr_ray_map(list(view), fov)
    info, passes = r.kerr_ray_map_info(), r.kerr_ray_map_passes()
    for n, (t, frame) in enumerate(rolls + ((rolls[1],) if swap else ())):
        if n == len(rolls):
            _set_scene(r, 37)                                # the map outlives a scene swap: it holds no scene
        r.render_from_kerr_ray_map_async(t_offset=t)
        got = _read(r)
        r.render_async(list(view), fov, frame=frame)
        want = _read(r)
        steps = r.counters()["ray_steps"]
        _assert_equal(got, want, f"{tag} t={t:g}" + (" swapped" if n == len(rolls) else ""))
        assert (want["disk"] > 0).any() and (want["bg"] > 0).any(), f"{tag}: a blank frame"
        assert int(passes["steps"].astype(np.int64).sum()) == info["ray_steps"] == steps, (tag, info["ray_steps"], steps)
    return info, passes


# ---- 1. a map frame is the marched Kerr frame ---------------------------------------------------------------------------------------
CASES = [(A, v, m, False) for A, v in ((0.6, KC.VIEWS[0]), (-0.9, KC.VIEWS[1]), (0.998, KC.VIEWS[0])) for m in ("model", "exact")] + \
        [(0.0, KC.VIEWS[0], "model", True)]


@pytest.mark.parametrize("A, view, redshift, force", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_map_frame_is_the_marched_frame(A, view, redshift, force, hip_lib):
    r = _mk(A, redshift, force)
    info, passes = _identity(r, view, KC.FOV, f"A={A} {view} {redshift}")
    r.close()
    assert info["built"] == 1 and info["spin"] == pytest.approx(A, abs=1e-7) and info["redshift"] == redshift
    assert info["crossings_stored"] == int(np.minimum(passes["crossings"], info["slots"]).sum()) > 0
    assert set(np.unique(passes["status"])) <= {0, 1, 2} and (passes["status"] == 1).any() and (passes["status"] == 0).any()


# ---- 2. ragged frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", KC.RAGGED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("redshift", ["model", "exact"])
def test_ragged_frames(size, redshift, hip_lib):
    w, h = size
    r = _mk(0.9, redshift, width=w, height=h)
    info, passes = _identity(r, KC.VIEWS[1], KC.FOV, f"{w}x{h} {redshift}", rolls=ROLLS[:2], swap=False)
    r.close()
    hits, n, K = passes["hits"], passes["crossings"], info["slots"]
    assert hits.shape == (K, h, w, 5) and passes["escape_dir"].shape == (h, w, 3)
    for c in range(K):                                       # no record beyond a pixel's crossings, no direction without an escape
        assert not hits[c][n <= c].any(), f"slot {c}: a record beyond the pixel's crossings"
    assert not passes["escape_dir"][passes["status"] != 1].any()
    esc = passes["escape_dir"][passes["status"] == 1].astype(np.float64)
    assert np.allclose(np.linalg.norm(esc, axis=-1), 1.0, atol=1e-5)


# ---- 3. the overflow path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("redshift", ["model", "exact"])
def test_overflow_pixels_are_marched(redshift, hip_lib):
    e = KC.CROSSINGS[0]                                      # A 0.998, fov 40, r_inner 0.7: rays that cross the annulus twice
    r = _mk(e.A, redshift, r_disk_inner=e.r_inner)
    for slots in (1, 4, 8):
        r.set_option("raymap_slots", slots)
        info, passes = _identity(r, e.view, e.fov, f"slots {slots} {redshift}", rolls=ROLLS[:2], swap=False)
        assert info["slots"] == slots and info["overflow_pixels"] == int((passes["crossings"] > slots).sum())
        if slots == 1:
            assert info["overflow_pixels"] > 0, "no pixel with two crossings: the fix kernel did not run"
    r.close()


# ---- 4. turned views: the rotation alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A, redshift, k", [(0.6, "model", 37), (0.6, "exact", 301), (-0.9, "model", 1), (-0.9, "exact", 37)])
def test_the_rotation_alone(A, redshift, k, hip_lib):
    """e_rot: the map frame turned to camera k under the scene S against the angle-0 map frame under S rolled by -k columns -- the
    same stored rays; only the roundings of the turn (and of the samplers' own coordinates) separate them.  The bar e_noise comes
    from code this map does not touch: the marched Kerr frame at camera k under S against the marched Kerr frame at camera 0 under
    the rolled S, two marches of symmetric views.  k is no multiple of 128 (a quarter turn is exact)."""
    assert k % 128 != 0
    r = _mk(A, redshift)
    r.build_kerr_ray_map(_cam(0), KC.FOV)
    r.render_from_kerr_ray_map_async(t_offset=0.5, skip_bloom=True)
    plain = _read(r, ("bg", "disk"), u8=False)
    r.render_from_kerr_ray_map_async(t_offset=0.5, cam_pos=_cam(0), skip_bloom=True)
    angle0 = _read(r, ("bg", "disk"), u8=False)
    _assert_equal(angle0, plain, "angle 0 through render_view")
    r.render_from_kerr_ray_map_async(t_offset=0.5, cam_pos=_cam(k), skip_bloom=True)
    turned = _read(r, ("bg", "disk"), u8=False)
    r.render_async(_cam(k), KC.FOV, frame=5, skip_bloom=True)
    march_k = _read(r, ("bg", "disk"), u8=False)
    _set_scene(r, k)
    r.render_from_kerr_ray_map_async(t_offset=0.5, skip_bloom=True)
    rolled = _read(r, ("bg", "disk"), u8=False)
    r.render_async(_cam(0), KC.FOV, frame=5, skip_bloom=True)
    march_0_rolled = _read(r, ("bg", "disk"), u8=False)
    r.close()
    for name in ("bg", "disk"):
        e_rot, e_noise = KC.rmse(turned[name], rolled[name]), KC.rmse(march_k[name], march_0_rolled[name])
        far = int((np.abs(turned[name] - rolled[name]).max(axis=2) > 0.05).sum())
        print(f"\n[kerr map rotation] A={A} {redshift} k={k} {name}: e_rot {e_rot:.3g}, e_noise {e_noise:.3g}, pixels beyond 0.05: {far}")
        assert np.isfinite(turned[name]).all()
        assert e_rot <= e_noise, f"{name}: e_rot {e_rot} above e_noise {e_noise}"
        assert far == 0, f"{name}: {far} pixels beyond 0.05"
        assert (turned[name] != angle0[name]).any(), "the turned frame is the angle-0 frame: the test cannot fail"


# ---- 5. a turned view against binary64 ----------------------------------------------------------------------------------------------
def _probe_scene():
    sky = np.ones((16, 32, 3), dtype=np.float32)
    tex = np.ones((8, 16, 4), dtype=np.float32)
    tex[..., 3] = PROBE_ALPHA
    return sky, tex


def _same(sky, n, ref):
    """Pixels whose fate and crossing count (n: crossings of a ray that reached the sky; of a dark one, whether it crossed at all)
    are the reference's: tests/test_gpu_kerr.py's rule."""
    ref_sky = ref["fate"] == 1
    same = sky == ref_sky
    same &= np.where(sky & ref_sky, n == ref["n_hits"], True)
    same &= np.where(~sky & ~ref_sky, (n > 0) == (ref["n_hits"] > 0), True)
    return same


@pytest.mark.parametrize("redshift", ["model", "exact"])
def test_turned_map_frame_against_binary64(redshift, hip_lib):
    """Frame 7 of a 24-frame orbit of pov (6, 0, 0.5) around the hole of A = 0.6: the turned map frame may be no further from the
    binary64 reference of that view than 1.5 x the marched Kerr frame of that view is, per layer, over the pixels whose fate and
    crossing count are the reference's; at most FATE_SHARE of either frame's pixels are left out."""
    A, view = 0.6, tuple(_cam(7, 24))
    case = KC.Edge(A, view, redshift=redshift)
    d32, share32 = KC.float32_distance(case)
    assert share32 <= FATE_SHARE, f"the view sits on a discontinuity: float32 against float64 differs on {share32:.3%}"
    ref = KC.edge_reference(case, np.float64)
    r = _mk(A, redshift)
    r.build_kerr_ray_map(_cam(0, 24), KC.FOV)
    passes = r.kerr_ray_map_passes()
    r.render_from_kerr_ray_map_async(t_offset=0.0, cam_pos=list(view), skip_bloom=True)
    got = _read(r, u8=False)
    r.render_async(list(view), KC.FOV, skip_bloom=True)
    marched = _read(r, u8=False)
    r.close()
    p = _mk(A, redshift, scene=_probe_scene())               # the marched frame's fates and crossings, from a probe frame
    p.render_async(list(view), KC.FOV, skip_bloom=True)
    probe = _read(p, ("bg", "disk"), u8=False)
    p.close()
    bg = probe["bg"][..., 0].astype(np.float64)
    m_sky = bg > 0
    m_n = np.where(m_sky, np.rint(-np.log2(np.where(m_sky, bg, 1.0))), (probe["disk"].max(axis=2) > 0)).astype(np.int64)
    same_map, same_march = _same(passes["status"] == 1, passes["crossings"], ref), _same(m_sky, m_n, ref)
    e_map, e_march = KC.distance(got, ref, same_map), KC.distance(marched, ref, same_march)
    out_map, out_march = float((~same_map).mean()), float((~same_march).mean())
    print(f"\n[kerr map binary64] {redshift}: map-binary64 {e_map} (left out {out_map:.3%}), marched-binary64 {e_march} (left out {out_march:.3%}), "
          f"float32 reference {d32} ({share32:.3%})")
    assert out_map <= FATE_SHARE and out_march <= FATE_SHARE
    for layer in ("bg", "disk", "final"):
        assert e_map[layer] <= 1.5 * e_march[layer], f"{layer}: map {e_map[layer]:.3g} over 1.5 x marched {e_march[layer]:.3g}"


# ---- 6. state and refusals ----------------------------------------------------------------------------------------------------------
def _refused(r, exc, words, call):
    """`call` raises exc with every word in the message, launches nothing, and the context renders as before."""
    before = r.counters()["frames_timed"]
    with pytest.raises(exc) as e:
        call()
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert r.counters()["frames_timed"] == before


def test_state_and_refusals(hip_lib):
    from bhr_amd import HipRenderer, _lib
    view = list(KC.VIEWS[0])
    plain = _mk(0.0)                                         # no spin: the Schwarzschild map is the call
    _refused(plain, AssertionError, ("bhr_kerr_raymap_build", "bhr_raymap_build"), lambda: plain.build_kerr_ray_map(view, KC.FOV))
    plain.build_ray_map(view, KC.FOV, skip_differentials=True)
    plain.render_from_ray_map_async(frame=3)
    schw = _read(plain)

    r = _mk(0.6)
    r.render_async(view, KC.FOV)
    want = _read(r)
    _refused(r, AssertionError, ("bhr_kerr_raymap_render", "bhr_kerr_raymap_build"), lambda: r.render_from_kerr_ray_map_async())
    with pytest.raises(AssertionError):
        r.kerr_ray_map_passes()
    assert r.kerr_ray_map_info()["built"] == 0
    with pytest.raises(ValueError) as e:                     # the Schwarzschild map under a spin is refused as ever
        r.build_ray_map(view, KC.FOV)
    assert "spin" in str(e.value) and "ray map" in str(e.value)
    r.set_option("raymap_supersample", 2)
    _refused(r, ValueError, ("bhr_kerr_raymap_build", "raymap_supersample"), lambda: r.build_kerr_ray_map(view, KC.FOV))
    r.set_option("raymap_supersample", 1)
    _refused(r, ValueError, ("bhr_kerr_raymap_build", "flags"), lambda: _lib.check(r._lib.bhr_kerr_raymap_build(r._ctx, r.camera_uniforms(view, KC.FOV), 1)))

    r.build_kerr_ray_map(view, KC.FOV)
    n0 = r.counters()["frames_timed"]
    r.render_from_kerr_ray_map_async()
    _assert_equal(_read(r), want, "the map frame")
    assert r.counters()["frames_timed"] == n0 + 1            # one timing-ring entry, like any frame
    # a camera that is no turn about z: another height, another distance, the build's position with another field of view
    for pos in ([6.0, 0.0, 0.7], [5.0, 0.0, 0.5]):
        _refused(r, ValueError, ("bhr_kerr_raymap_render_view",), lambda: r.render_from_kerr_ray_map_async(cam_pos=pos))
    cam = r.camera_uniforms(view, 60.0)
    _refused(r, ValueError, ("bhr_kerr_raymap_render_view",), lambda: _lib.check(r._lib.bhr_kerr_raymap_render_view(r._ctx, cam, 0)))
    _refused(r, ValueError, ("bhr_kerr_raymap_render", "flags"), lambda: _lib.check(r._lib.bhr_kerr_raymap_render(r._ctx, 0.0, _lib.FORCE_FAST)))
    _refused(r, ValueError, ("bhr_kerr_raymap_render", "t_offset"), lambda: r.render_from_kerr_ray_map_async(t_offset=float("nan")))
    _refused(r, ValueError, ("bhr_kerr_raymap_render_view", "t_offset"),
             lambda: r.render_from_kerr_ray_map_async(t_offset=float("inf"), cam_pos=view))
    # the context's spin or redshift mode is no longer the build's: the message names both values
    r.set_spin(0.5)
    _refused(r, AssertionError, ("bhr_kerr_raymap_render", "0.6", "0.5"), lambda: r.render_from_kerr_ray_map_async())
    r.set_spin(0.6)
    r.set_redshift("exact")
    _refused(r, AssertionError, ("bhr_kerr_raymap_render", "model", "exact"), lambda: r.render_from_kerr_ray_map_async())
    _refused(r, AssertionError, ("bhr_kerr_raymap_render_view", "model", "exact"), lambda: r.render_from_kerr_ray_map_async(cam_pos=view))
    r.set_redshift("model")
    r.render_from_kerr_ray_map_async()                       # back at the build's setting the map serves again
    _assert_equal(_read(r), want, "the map frame after the refusals")
    r.render_async(view, KC.FOV)
    _assert_equal(_read(r), want, "the marched frame after the refusals")
    r.free_kerr_ray_map()
    assert r.kerr_ray_map_info()["built"] == 0
    _refused(r, AssertionError, ("bhr_kerr_raymap_render",), lambda: r.render_from_kerr_ray_map_async())
    r.close()

    # a row-block context takes neither a spin nor a Kerr map
    sky, tex = _scene()
    rows = HipRenderer(KC.W, KC.H, sky, tex, math="strict", rows=(0, KC.H // 2), **KW)
    with pytest.raises(ValueError) as e:
        rows.build_kerr_ray_map(view, KC.FOV)
    assert "bhr_kerr_raymap_build" in str(e.value) and "whole-frame" in str(e.value)
    rows.close()

    # the Schwarzschild map of the other context has seen none of this
    plain.render_from_ray_map_async(frame=3)
    _assert_equal(_read(plain), schw, "the Schwarzschild map frame")
    assert plain.ray_map_info()["built"] == 1 and plain.kerr_ray_map_info()["built"] == 0
    plain.close()


# ---- 7. video -----------------------------------------------------------------------------------------------------------------------
def _video(tmp_path, name, orbit, spin_map, resume=False, renderer=None):
    from bhr_amd import drivers
    sky, tex = _scene()
    pov = list(KC.VIEWS[0])
    r = renderer or _mk(0.6, width=64, height=40)
    out = str(tmp_path / name / "v.mp4")
    drivers.render_video(r, 64, 40, n_frames=6, fps=24, output_path=out, fov=KC.FOV, static_cam_pos=pov, orbit=orbit, resume=resume,
                         video_stream="off", assemble=False, spin_map=spin_map)
    d = drivers._frames_dir(out)
    frames = [open(os.path.join(d, f"frame_{f:04d}.png"), "rb").read() for f in range(6)]
    with open(os.path.join(d, "progress.json")) as fh:
        rec = json.load(fh)
    return r, frames, rec


def _decode(png):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB"), dtype=np.float64) / 255.0


@pytest.mark.parametrize("orbit", [False, True], ids=["still", "orbit"])
def test_video(orbit, tmp_path, hip_lib, capsys):
    r, marched, rec0 = _video(tmp_path, "marched", orbit, False)
    assert "spin_map" not in rec0["params"]
    r.close()
    r, mapped, rec1 = _video(tmp_path, "mapped", orbit, True)
    assert rec1["params"]["spin_map"] is True and rec1["completed"] == list(range(6))
    assert r.kerr_ray_map_info()["built"] == 0               # freed at the end
    assert mapped[0] == marched[0]
    if not orbit:
        assert mapped == marched                             # byte-identical frame files
    else:
        for f in range(1, 6):
            e = KC.rmse(_decode(mapped[f]), _decode(marched[f]))
            print(f"\n[kerr map video] orbit frame {f}: RMSE to the marched frame {e:.3g}")
            assert e <= 1.0 / 255.0 and mapped[f] != mapped[0]
    # a resume with the same setting takes the frames up; with the other setting it starts over
    capsys.readouterr()
    _video(tmp_path, "mapped", orbit, True, resume=True, renderer=r)
    assert "Resuming: 6/6" in capsys.readouterr().out
    _, again, rec2 = _video(tmp_path, "mapped", orbit, False, resume=True, renderer=r)
    assert "starting over" in capsys.readouterr().out and "spin_map" not in rec2["params"]
    assert again == marched
    r.close()


# ---- 7. both maps through one context -------------------------------------------------------------------------------------------------
def test_both_maps_through_one_context(hip_lib):
    """A context holds a Schwarzschild map and a Kerr map side by side, and building, rebuilding or freeing one leaves the other
    as it was: its info field for field, its frames bit for bit.  The smallest ragged frame with no side a multiple of 8; with one
    slot per pixel both maps have pixels on the overflow list and pixels off it, so the fix launch of both kinds runs."""
    w, h = min((s for s in KC.RAGGED_SIZES if s[0] % 8 and s[1] % 8), key=lambda s: s[0] * s[1], default=(61, 37))
    view, fov = list(KC.VIEWS[0]), KC.FOV
    r = _mk(0.0, width=w, height=h)
    # 1. the Schwarzschild map at spin 0, one slot
    r.set_option("raymap_slots", 1)
    r.build_ray_map(view, fov, skip_differentials=True)
    r.render_from_ray_map_async(frame=3)
    S = _read(r)
    r.render_async(view, fov, frame=3, skip_differentials=True)
    _assert_equal(S, _read(r), "the Schwarzschild map's frame")
    schw = r.ray_map_info()
    assert schw["built"] == 1 and schw["slots"] == 1 and 0 < schw["overflow_pixels"] < w * h, schw
    # 2. the Kerr map beside it, under both redshifts
    r.set_spin(0.6)
    for redshift in ("model", "exact"):
        r.set_redshift(redshift)
        r.build_kerr_ray_map(view, fov)
        r.render_from_kerr_ray_map_async()
        K = _read(r)
        r.render_async(view, fov)
        _assert_equal(K, _read(r), f"the Kerr map's frame, {redshift} redshift")
        kerr1 = r.kerr_ray_map_info()
        assert kerr1["built"] == 1 and kerr1["slots"] == 1 and kerr1["redshift"] == redshift and 0 < kerr1["overflow_pixels"] < w * h, kerr1
        # 3. the Schwarzschild map is as it was
        assert r.ray_map_info() == schw
    # 4. four slots: three more records of 5 floats per pixel, and nothing else
    r.set_option("raymap_slots", 4)
    r.build_kerr_ray_map(view, fov)
    kerr4 = r.kerr_ray_map_info()
    assert kerr4["slots"] == 4 and kerr4["device_bytes"] - kerr1["device_bytes"] == 3 * 5 * w * h * 4
    r.render_from_kerr_ray_map_async()
    _assert_equal(_read(r), K, "the Kerr map's frame, four slots")
    assert r.ray_map_info() == schw
    # 5. the Kerr map freed, the Schwarzschild map stays
    r.free_kerr_ray_map()
    gone = r.kerr_ray_map_info()
    assert gone["built"] == 0 and gone["device_bytes"] == 0
    assert r.ray_map_info() == schw
    # 6. ... and still gives its frame once the spin is off
    r.set_redshift("model")
    r.set_spin(0.0)
    r.render_from_ray_map_async(frame=3)
    _assert_equal(_read(r), S, "the Schwarzschild map's frame behind the Kerr map's life")
    # 7. both gone
    r.free_ray_map()
    assert r.ray_map_info()["built"] == 0 and r.kerr_ray_map_info()["built"] == 0
    r.close()


# ---- 8. the launchers both kinds share, alternating on one context ------------------------------------------------------------------------
def test_shared_launchers_alternate_between_the_kinds(hip_lib):
    """The fused shutter launch and the Stokes pass of both map kinds go through one launcher each, which takes the kind from the
    frame's variant.  One context alternates between the kinds: Schwarzschild, Kerr under either redshift, Schwarzschild again.
    Every fused shutter frame is bit for bit the frame of its own unfused route, and the first and last Schwarzschild frames are
    equal; with a polarisation and a Kerr polarisation set, the Stokes planes of each kind are those of a context that only ever
    held that kind.  27 x 19 (partial tiles on both sides), three samples, eight slots: no map has overflow pixels, so the
    shutter frames take the fused launch -- counted under option "shutter_timing", which brackets the accumulation launches the
    fused route has none of."""
    from bhr_amd import drivers
    w, h, n, fov = 27, 19, 3, KC.FOV
    u = drivers.shutter_times(5, 0.5, n)
    pos, toff = [_cam(t) for t in u], [(t - 5) * 0.1 for t in u]
    layers = ("final", "bg", "disk")

    def both_routes(r, render, option, tag):
        got = {}
        for fused, launches in ((1, 0), (0, n)):
            r.set_option(option, fused)
            render(toff, pos, fov)
            got[fused] = _read(r, layers)
            assert r.shutter_timing()["launches"] == launches, (tag, fused)
        r.set_option(option, 1)
        _assert_equal(got[1], got[0], f"{tag}: the fused launch against the sample-by-sample route")
        assert (got[1]["disk"] > 0).any() and (got[1]["bg"] > 0).any(), f"{tag}: a blank frame"
        return got[1]

    r = _mk(0.0, width=w, height=h)
    r.set_option("raymap_slots", 8)
    r.set_option("shutter_timing", 1)
    r.build_ray_map(_cam(0), fov)
    assert r.ray_map_info()["overflow_pixels"] == 0
    first = both_routes(r, r.render_shutter_from_ray_map_async, "raymap_shutter_fused", "Schwarzschild")
    r.set_spin(0.6)
    for redshift in ("model", "exact"):
        r.set_redshift(redshift)
        r.build_kerr_ray_map(_cam(0), fov)
        assert r.kerr_ray_map_info()["overflow_pixels"] == 0
        K = both_routes(r, r.render_shutter_from_kerr_ray_map_async, "kerr_raymap_shutter_fused", f"Kerr, {redshift} redshift")
        assert (K["disk"] != first["disk"]).any()
    r.set_redshift("model")
    r.set_spin(0.0)
    _assert_equal(both_routes(r, r.render_shutter_from_ray_map_async, "raymap_shutter_fused", "Schwarzschild again"), first,
                  "the Schwarzschild shutter frame behind the Kerr ones")
    r.close()

    # the Stokes pass: the planes and the cell means of a map frame of either kind
    view, t, field, kerr_field = list(KC.VIEWS[0]), 0.7, "toroidal", (0.3, 0.8, 0.5)

    def planes(r, kerr):
        (r.render_from_kerr_ray_map_async if kerr else r.render_from_ray_map_async)(t_offset=t, skip_bloom=True)
        S, cells = r.stokes(), r.stokes_cells()
        assert S[0].any() and S[1].any() and cells.any()
        return S, cells

    def same(got, want, tag):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{tag}: the Stokes planes differ"

    alone = {}
    s = _mk(0.0, width=w, height=h)
    s.set_polarization(field, 0.7, 8)
    s.build_ray_map(view, fov)
    alone["schwarzschild"] = planes(s, False)
    s.close()
    k = _mk(0.6, width=w, height=h)
    k.set_kerr_polarization(kerr_field, 0.7, 8)
    for redshift in ("model", "exact"):
        k.set_redshift(redshift)
        k.build_kerr_ray_map(view, fov)
        alone[redshift] = planes(k, True)
    k.close()

    r = _mk(0.0, width=w, height=h)
    r.set_polarization(field, 0.7, 8)
    r.build_ray_map(view, fov)
    same(planes(r, False), alone["schwarzschild"], "Schwarzschild")
    r.set_spin(0.6)
    r.set_kerr_polarization(kerr_field, 0.7, 8)
    for redshift in ("model", "exact"):
        r.set_redshift(redshift)
        r.build_kerr_ray_map(view, fov)
        same(planes(r, True), alone[redshift], f"Kerr, {redshift} redshift")
    r.set_redshift("model")
    r.set_spin(0.0)
    same(planes(r, False), alone["schwarzschild"], "Schwarzschild behind the Kerr frames")
    r.close()
