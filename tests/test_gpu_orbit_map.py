"""One ray map for a whole orbit (bhr_raymap_render_view; include/bhr.h states the contract): with a disk that is not tilted, the
orbit's turn of the camera about z is a symmetry of everything a ray's path depends on, so a frame of the orbit is shaded from
the map of frame 0 with the stored records turned by the orbit angle.  Such a frame is the strict march of the BUILD view's
rays: bit for bit the map frame at angle 0, and elsewhere as far from the strict march of its view as two strict marches of
symmetric views are from each other.

Scenes: scenes.analytic_skybox() and scenes.noisy_disk(), both 512 columns wide, so that at the orbit angles 2 pi k / 512 "the
frame-0 rays turned by the angle" is also "the frame-0 rays under the sky and the texture rolled by -k columns" -- the second
needs no rotation code.  pov (6, 0, 0.5), fov 90, frame 5.  Frames: 96 x 54 (the hole's image, rays with two crossings), 21 x 13
(partial tiles on both sides), 24 x 15 anti-aliased (records with differentials)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POV, FOV, FRAME = (6.0, 0.0, 0.5), 90.0, 5
VIEWS = {
    "ring": dict(W=96, H=54, kw=()),
    "odd": dict(W=21, H=13, kw=()),
    "aa": dict(W=24, H=15, kw=(("anti_alias", "lod_radius"), ("disk_tilt", 0.0))),
    "ring_aa": dict(W=96, H=54, kw=(("anti_alias", "lod_radius"), ("disk_tilt", 0.0))),
}
LAYERS = ("final", "bg", "disk", "blur")


def _cam(k, n=512, pov=POV):
    from bhr_amd.camera import orbit_position
    return [float(v) for v in orbit_position(list(pov), k, n)]


@functools.lru_cache(maxsize=None)
def _scene(roll=0):
    """The scene, its sky and texture rolled by -roll columns: what the frame-0 rays see in place of a turn by 2 pi roll / 512."""
    from bhr_amd import scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    assert sky.shape[1] == tex.shape[1] == 512
    sky, tex = np.ascontiguousarray(np.roll(sky, -roll, axis=1)), np.ascontiguousarray(np.roll(tex, -roll, axis=1))
    sky.setflags(write=False)
    tex.setflags(write=False)
    return sky, tex


def _mk(view, roll=0, **kw):
    from bhr_amd import HipRenderer
    v = VIEWS[view]
    sky, tex = _scene(roll)
    return HipRenderer(v["W"], v["H"], sky, tex, math="strict", **dict(v["kw"]), **kw)


def _set_scene(r, roll):
    from bhr_amd import _lib
    sky, tex = _scene(roll)
    _lib.check(r._lib.bhr_set_skybox(r._ctx, _lib.fptr(sky), sky.shape[0], sky.shape[1]))
    r.update_disk_texture(tex)


def _read(r, names=LAYERS):
    from bhr_amd import _lib
    ids = dict(final=_lib.LAYER_FINAL, bg=_lib.LAYER_BG, disk=_lib.LAYER_DISK, blur=_lib.LAYER_BLUR)
    out = {k: r.read_layer(ids[k]) for k in names}
    out["u8"] = r.read_final_u8()
    return out


def _rmse(a, b):
    """Per channel, in binary64."""
    return np.sqrt(np.mean((a.astype(np.float64) - b) ** 2, axis=(0, 1)))


def _assert_equal(got, want, tag, names=LAYERS + ("u8",)):
    for k in names:
        bad = int((got[k] != want[k]).any(axis=-1).sum())
        assert bad == 0, f"{tag} {k}: {bad} pixels differ (max |d| {np.abs(got[k].astype(np.float64) - want[k]).max():.3g})"


# ---- 1. angle 0 is the map frame --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["ring", "odd", "aa"])
def test_angle_zero_is_the_map_frame(view, hip_lib):
    r = _mk(view)
    r.build_ray_map(_cam(0), FOV)
    r.render_from_ray_map_async(frame=FRAME)
    want = _read(r)
    r.render_from_ray_map_async(frame=FRAME, cam_pos=_cam(0), fov=FOV)
    got = _read(r)
    r.render_from_ray_map_async(frame=FRAME, cam_pos=_cam(37), fov=FOV)
    turned = _read(r)
    r.close()
    _assert_equal(got, want, f"{view} angle 0")
    assert (want["disk"] > 0).any() and (want["bg"] > 0).any()
    assert (turned["bg"] != want["bg"]).any() and (turned["disk"] != want["disk"]).any()      # the keyword is not ignored


# ---- 2. the rotation alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view,k", [("ring", 1), ("ring", 37), ("ring", 301), ("odd", 37), ("aa", 48), ("aa", 208)])
def test_the_rotation_alone(view, k, hip_lib):
    """e_rot: the frame from the map turned to camera k under the scene S, against bhr_raymap_render of the same map under S
    rolled by -k columns.  Both shade the same stored rays; only the roundings of the rotation (and of the samplers' own
    coordinates) separate them.  The bar, e_noise, is measured here from code the rotation does not touch: the strict bhr_render
    at camera k under S against the strict bhr_render at camera 0 under the rolled S -- two strict marches of symmetric views.
    k is no multiple of 128 (a quarter turn is exact); the anti-aliased k are multiples of 16, so the mip levels roll too."""
    from bhr_amd import _lib
    assert k % 128 != 0 and (view != "aa" or k % 16 == 0)
    r = _mk(view)
    r.build_ray_map(_cam(0), FOV)
    assert r.ray_map_info()["diff"] == (1 if view == "aa" else 0)
    r.render_from_ray_map_async(frame=FRAME, cam_pos=_cam(k), fov=FOV, skip_bloom=True)
    turned = _read(r, ("bg", "disk"))
    r.render_from_ray_map_async(frame=FRAME, cam_pos=_cam(0), fov=FOV, skip_bloom=True)
    angle0 = _read(r, ("bg", "disk"))
    r.render_async(_cam(k), FOV, frame=FRAME, skip_bloom=True, math="strict")
    march_k = _read(r, ("bg", "disk"))
    _set_scene(r, k)
    r.render_from_ray_map_async(frame=FRAME, skip_bloom=True)
    rolled = _read(r, ("bg", "disk"))
    r.render_async(_cam(0), FOV, frame=FRAME, skip_bloom=True, math="strict")
    march_0_rolled = _read(r, ("bg", "disk"))
    r.close()
    for name in ("bg", "disk"):
        e_rot, e_noise = _rmse(turned[name], rolled[name]), _rmse(march_k[name], march_0_rolled[name])
        far = int((np.abs(turned[name] - rolled[name]).max(axis=2) > 0.05).sum())
        far_noise = int((np.abs(march_k[name] - march_0_rolled[name]).max(axis=2) > 0.05).sum())
        print(f"\n[orbit map rotation] {view} k={k} {name}: e_rot {e_rot.max():.3g} {e_rot}, e_noise {e_noise.max():.3g} {e_noise}, "
              f"pixels beyond 0.05: {far} (marches: {far_noise})")
        assert np.isfinite(turned[name]).all()
        assert (e_rot <= e_noise).all(), f"{view} k={k} {name}: e_rot {e_rot} above e_noise {e_noise}"
        assert far == 0, f"{view} k={k} {name}: {far} pixels beyond 0.05"
        assert (turned[name] != angle0[name]).any(), "the turned frame is the angle-0 frame: the test cannot fail"


# ---- 3. against binary64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["ring", "ring_aa"])
@pytest.mark.parametrize("f", [7, 17])
def test_turned_map_frame_against_binary64(view, f, oracle, hip_lib):
    """The project's yardstick for two f32 evaluations of one view (test_gpu_fuzz.py, the telephoto views), with no pixel set
    aside: the turned-map frame may be no further from the oracle's binary64 build at that camera than 1.5 x the strict march of
    that camera is, with a floor of 6e-5.  Angles that are not aligned with the texels: frames 7 and 17 of a 24-frame orbit."""
    v = VIEWS[view]
    cam = _cam(f, 24)
    r = _mk(view)
    r.build_ray_map(_cam(0, 24), FOV)
    r.render_from_ray_map_async(frame=FRAME, cam_pos=cam, fov=FOV, skip_bloom=True)
    got = _read(r, ("bg", "disk"))
    r.render_async(cam, FOV, frame=FRAME, skip_bloom=True, math="strict")
    strict = _read(r, ("bg", "disk"))
    r.close()
    sky, tex = _scene(0)
    ora = oracle.OracleRenderer(v["W"], v["H"], sky, tex, fast="f64", **dict(v["kw"]))
    ref = dict(zip(("bg", "disk"), (x.transpose(1, 0, 2) for x in ora.march(cam, FOV, frame=FRAME))))
    for name in ("bg", "disk"):
        e_map, e_strict = float(_rmse(got[name], ref[name]).max()), float(_rmse(strict[name], ref[name]).max())
        far = int((np.abs(got[name] - strict[name]).max(axis=2) > 0.05).sum())
        print(f"\n[orbit map binary64] {view} frame {f} {name}: map-binary64 {e_map:.3g}, strict-binary64 {e_strict:.3g}, "
              f"map-strict {float(_rmse(got[name], strict[name]).max()):.3g}, pixels beyond 0.05: {far}")
        assert e_map <= max(6e-5, 1.5 * e_strict), (view, f, name, e_map, e_strict)
        assert far == 0, (view, f, name, far)


# ---- 4. overflow pixels are marched at the frame's camera ---------------------------------------------------------------------
def test_overflow_pixels_are_the_strict_march_of_the_frames_camera(hip_lib):
    k = 37
    r = _mk("ring", options={"raymap_slots": 1})
    r.build_ray_map(_cam(0), FOV)
    over = r.ray_map_passes()["crossings"] > 1
    assert r.ray_map_info()["overflow_pixels"] == int(over.sum()) > 0
    r.render_from_ray_map_async(frame=FRAME, cam_pos=_cam(k), fov=FOV)
    got = _read(r)
    r.render_async(_cam(k), FOV, frame=FRAME, math="strict")
    strict_k = _read(r)
    r.render_async(_cam(0), FOV, frame=FRAME, math="strict")
    strict_0 = _read(r)
    r.close()
    for name in ("bg", "disk"):
        np.testing.assert_array_equal(got[name][over], strict_k[name][over])
    assert (strict_k["disk"][over] != strict_0["disk"][over]).any()      # ... and not the march of the build camera
    assert (got["disk"][~over] != strict_k["disk"][~over]).any()         # the other pixels are shaded from turned records


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_context_usable(hip_lib):
    from bhr_amd import HipRenderer, _lib
    lib = hip_lib
    view, k = "odd", 37
    r = _mk(view)
    cam_k = r.camera_uniforms(_cam(k), FOV, FRAME)

    def refused(ctx, cam, flags, code, word=None):
        rc = lib.bhr_raymap_render_view(ctx, C.byref(cam) if cam is not None else None, flags)
        assert rc == code, (rc, lib.bhr_last_error())
        assert b"bhr_raymap_render_view" in lib.bhr_last_error()
        if word is not None:
            assert word in lib.bhr_last_error(), lib.bhr_last_error()

    refused(r._ctx, cam_k, 0, _lib.BHR_ERR_STATE, b"no ray map")          # before a build
    r.build_ray_map(_cam(0), FOV)
    r.render_from_ray_map_async(frame=FRAME, cam_pos=_cam(k), fov=FOV)
    want = _read(r)

    def still_renders(ctx_r=r):
        before = ctx_r.counters()["frames_timed"]
        ctx_r.render_from_ray_map_async(frame=FRAME, cam_pos=_cam(k), fov=FOV)
        _assert_equal(_read(ctx_r), want, "after a refusal")
        return before

    frames = still_renders()

    def edited(**kw):
        cam = _lib.Camera.from_buffer_copy(cam_k)
        for name, value in kw.items():
            if isinstance(value, (list, tuple)):
                getattr(cam, name)[:] = list(value)
            else:
                setattr(cam, name, value)
        return cam

    pos = list(cam_k.pos)
    other_sense = r.camera_uniforms(_cam(-k), FOV, FRAME)
    bad_cams = [
        (r.camera_uniforms(_cam(k, pov=(5.0, 0.0, 0.5)), FOV, FRAME), None),              # another radius (and escape radius)
        (edited(pos=[pos[0] * 1.01, pos[1] * 1.01, pos[2]]), b"z axis"),                 # another radius, everything else equal
        (r.camera_uniforms(_cam(k, pov=(6.0, 0.0, 0.6)), FOV, FRAME), b"height"),        # another height
        (edited(pos=[pos[0], pos[1], pos[2] + 0.25]), b"height"),
        (r.camera_uniforms(_cam(k), 80.0, FRAME), b"pitch"),                              # another fov
        (r.camera_uniforms([0.0, 0.0, 6.0], FOV, FRAME), None),                           # on the axis
        (edited(pos=[0.0, 0.0, pos[2]]), b"z axis"),
        (edited(right=list(other_sense.right), up=list(other_sense.up), forward=list(other_sense.forward)), b"not a turn"),
        (edited(t_offset=float("nan")), b"t_offset"),
        (edited(t_offset=float("inf")), b"t_offset"),
    ]
    for cam, word in bad_cams:
        refused(r._ctx, cam, 0, _lib.BHR_ERR_INVALID, word)
    for flags in (_lib.SKIP_DIFFERENTIALS, _lib.PERSISTENT, _lib.FORCE_FAST, _lib.FORCE_HYBRID):
        refused(r._ctx, cam_k, flags, _lib.BHR_ERR_INVALID, b"flags")
    refused(r._ctx, None, 0, _lib.BHR_ERR_INVALID)
    refused(None, cam_k, 0, _lib.BHR_ERR_INVALID)
    assert r.counters()["frames_timed"] == frames + 1          # nothing but still_renders' frame was launched
    still_renders()
    with pytest.raises(ValueError):                            # the Python surface maps the codes as everywhere else
        r.render_from_ray_map_async(frame=FRAME, cam_pos=_cam(k, pov=(6.0, 0.0, 0.6)), fov=FOV)
    with pytest.raises(ValueError):
        r.render_from_ray_map_async(frame=FRAME, cam_pos=_cam(k))          # cam_pos without fov
    # supersampling and adaptive supersampling: the map stays and renders again once the setting is back
    for sampling in ((2, None), (2, 0.1)):
        r.set_supersample(*sampling)
        refused(r._ctx, cam_k, 0, _lib.BHR_ERR_STATE, b"supersampling")
        r.set_supersample(1)
        still_renders()
    r.free_ray_map()
    refused(r._ctx, cam_k, 0, _lib.BHR_ERR_STATE, b"no ray map")
    # a map built on the axis: the camera basis there does not turn with the position
    r.build_ray_map([0.0, 0.0, 6.0], FOV)
    refused(r._ctx, r.camera_uniforms([0.0, 0.0, 6.0], FOV, FRAME), 0, _lib.BHR_ERR_INVALID, b"z axis")
    r.render_from_ray_map_async(frame=FRAME)                   # bhr_raymap_render of that map is as it was
    assert np.isfinite(_read(r)["final"]).all()
    r.build_ray_map(_cam(0), FOV)
    still_renders()
    r.close()
    # a tilted disk: the settings of the ray map tests' "tilt" view
    sky, tex = _scene(0)
    t = HipRenderer(24, 15, sky, tex, math="strict", anti_alias="lod_radius", disk_tilt=20.0)
    t.build_ray_map([5.0, 2.0, 1.0], 80.0)
    t.render_from_ray_map_async(frame=FRAME)
    tilted = _read(t)
    before = t.counters()["frames_timed"]
    refused(t._ctx, t.camera_uniforms([5.0, 2.0, 1.0], 80.0, FRAME), 0, _lib.BHR_ERR_INVALID, b"tilted")
    assert t.counters()["frames_timed"] == before
    t.render_from_ray_map_async(frame=FRAME)
    _assert_equal(_read(t), tilted, "tilted: after the refusal")
    t.close()
    # a row-block context
    block = HipRenderer(21, 13, sky, tex, rows=(8, 13))
    refused(block._ctx, cam_k, 0, _lib.BHR_ERR_INVALID, b"whole-frame")
    block.close()


# ---- 6. driver ----------------------------------------------------------------------------------------------------------------
def test_orbit_video_from_one_ray_map(tmp_path, capsys, hip_lib):
    from PIL import Image
    from bhr_amd import drivers
    W, H, N = 48, 27, 6
    cam0, fov, speed = [6, 0, 0.5], 90, 0.1

    def video(out, **kw):
        r, _, _, _ = drivers.make_renderer(W, H, cam0, fov, n_stars=50, tex_w=256, tex_h=128, math="strict")
        try:
            drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=fov, static_cam_pos=cam0, orbit=True,
                                 disk_rotation_speed=speed, video_stream="off", assemble=False, **kw)
            assert r.ray_map_info()["built"] == 0            # the map is freed at the end
        finally:
            r.close()
        return drivers._frames_dir(out)

    def load(d, name):
        return np.asarray(Image.open(os.path.join(d, name)).convert("RGB"), dtype=np.float64) / 255.0

    d0 = video(str(tmp_path / "march" / "v.mp4"))
    d1 = video(str(tmp_path / "map" / "v.mp4"), orbit_map=True)
    names = [f"frame_{f:04d}.png" for f in range(N)]
    assert sorted(os.listdir(d0)) == sorted(os.listdir(d1)) == names + ["progress.json"]
    p0, p1 = (json.load(open(os.path.join(d, "progress.json")))["params"] for d in (d0, d1))
    assert "orbit_map" not in p0 and p1 == dict(p0, orbit_map=True)
    assert open(os.path.join(d0, names[0]), "rb").read() == open(os.path.join(d1, names[0]), "rb").read()
    first = load(d1, names[0])
    for name in names[1:]:
        got, want = load(d1, name), load(d0, name)
        assert (got != first).any(), name
        e = float(np.sqrt(np.mean((got - want) ** 2)))
        with capsys.disabled():
            print(f"\n[orbit map video] {name}: RMSE to the marched frame {e:.3g} ({e * 255:.3f} quantisation steps)")
        # two float frames closer than a quantisation step quantise at most one level apart; a wrong sense or a stale camera
        # gives 0.09 and more
        assert e <= 1.0 / 255.0, (name, e)
    # a resume under the other setting starts over: the frames become the marched ones
    capsys.readouterr()
    assert video(str(tmp_path / "map" / "v.mp4"), resume=True) == d1
    assert "starting over" in capsys.readouterr().out
    assert "orbit_map" not in json.load(open(os.path.join(d1, "progress.json")))["params"]
    for name in names:
        assert open(os.path.join(d0, name), "rb").read() == open(os.path.join(d1, name), "rb").read(), name
    with pytest.raises(ValueError, match="orbit_map"):
        video(str(tmp_path / "both" / "v.mp4"), orbit_map=True, ray_map=True)
    assert not os.path.exists(drivers._frames_dir(str(tmp_path / "both" / "v.mp4")))
