"""Point stars on the device (bhr_set_stars; include/bhr.h states the model, DESIGN.md 4 "Point stars"): the gather kernel's
star plane against the brute-force binary64 reference (tests/stars_ref.py) fed the DEVICE's own STATUS and ESCAPE_DIR planes,
its repeatability, the frame that adds the plane to the sky, turned views, the consumers behind the frame, and the refusals.

The bar of a plane: four times the float32 reference's own distance from the binary64 one on the same inputs, computed here, and
at least 1e-6 (distances are shares of the plane's maximum; stars_ref.distance says what a distance is); and at most 0.5 % of the
pixels further than 1e-3 of the maximum from the reference.

Scenes: scenes.analytic_skybox() and scenes.noisy_disk().  Frames 96 x 64 (crosses the gather's 15-pixel blocks and the shade's
8 x 8 tiles), 61 x 43 (ragged in both), one 5 x 3 (every triangle over the span)."""
import functools

import numpy as np
import pytest

import kerr_ref as K
import stars_ref as R

pytestmark = pytest.mark.gpu

FOV = 90.0
VIEWS = {"far": (6.0, 0.0, 0.5), "near": (3.0, 2.0, 0.3), "pole": (1.0, 0.0, 6.0)}


@functools.lru_cache(maxsize=None)
def _scene():
    from bhr_amd import scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    sky.setflags(write=False)
    tex.setflags(write=False)
    return sky, tex


def _mk(W=96, H=64, **kw):
    from bhr_amd import HipRenderer
    sky, tex = _scene()
    return HipRenderer(W, H, sky, tex, math="strict", **kw)


@functools.lru_cache(maxsize=None)
def _tables():
    from bhr_amd import skybox
    return skybox.sky_tables(2048, 1024, 42, 6000)


def _cam_dict(r, pos):
    """kerr_ref's camera dict from the uniforms the renderer hands the library."""
    c = r.camera_uniforms(list(pos), FOV, 0)
    f32 = np.float32
    return dict(pos=np.array(c.pos[:], dtype=f32), right=np.array(c.right[:], dtype=f32), up=np.array(c.up[:], dtype=f32),
                forward=np.array(c.forward[:], dtype=f32), pw=f32(c.pixel_width), ph=f32(c.pixel_height), width=r.width, height=r.height)


def _procedural(r, pos):
    from bhr_amd import stars
    cam = _cam_dict(r, pos)
    return stars.catalog_from_tables(_tables(), 2.0, float(cam["pw"]) * float(cam["ph"]))


def _synthetic():
    """Poles, the phi = 0 seam from both sides, duplicates, and 3000 stars over the whole sphere."""
    rng = np.random.default_rng(11)
    z = rng.uniform(-1, 1, 3000)
    phi = rng.uniform(0, 2 * np.pi, 3000)
    s = np.sqrt(1 - z * z)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=-1)
    eps = 1e-6
    seam_t = np.linspace(0.05, np.pi - 0.05, 40)
    seam = [np.stack([np.sin(seam_t) * np.cos(p), np.sin(seam_t) * np.sin(p), np.cos(seam_t)], axis=-1) for p in (0.0, 2 * np.pi - eps, eps)]
    polar_t = np.array([0.0, 1e-4, 1e-2, np.pi - 1e-2, np.pi - 1e-4, np.pi])
    polar = np.stack([np.sin(polar_t) * np.cos(1.0), np.sin(polar_t) * np.sin(1.0), np.cos(polar_t)], axis=-1)
    d = np.concatenate([d, *seam, polar, polar, d[:50]])            # the poles and 50 stars twice
    return d, rng.uniform(0.1, 1.0, (len(d), 3)) * 1e-4


def _as_device(dirs, flux):
    """The catalogue as the library holds it: f32 in, normalized in binary64, rounded once."""
    d = np.asarray(dirs, dtype=np.float64).astype(np.float32).astype(np.float64)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    return d, np.asarray(flux, dtype=np.float64).astype(np.float32)


def _references(r, pos, dirs, flux, angle=0.0, **kw):
    """(S64, S32): the binary64 and the float32 reference planes on the device's own map planes; `angle`: the catalogue turned
    about z on the host in binary64 (a view turned by -angle)."""
    p = r.ray_map_passes()
    cam = _cam_dict(r, pos)
    d, f = _as_device(dirs, flux)
    if angle:
        d = R.turn_z(d.astype(np.float64), angle)
    S64 = R.star_plane(p["status"], p["escape_dir"], K.pixel_rays(cam, np.float64), d, f, **kw)
    S32 = R.star_plane(p["status"], p["escape_dir"], K.pixel_rays(cam, np.float32), d.astype(np.float32), f, dtype=np.float32, **kw)
    return S64, S32


def _check_plane(got, S64, S32, tag):
    own, dev = R.distance(S32, S64), R.distance(got, S64)
    bar = max(4.0 * own, 1e-6)
    share = R.outlier_share(got, S64)
    print(f"{tag}: device distance {dev:.3e}, float32 reference {own:.3e}, bar {bar:.3e}; share beyond 1e-3 of the maximum {share:.5f} "
          f"(float32 reference {R.outlier_share(S32, S64):.5f}); largest difference {np.abs(got - S64).max() / S64.max():.3e} of the maximum")
    assert S64.max() > 0 and np.isfinite(got).all() and (got >= 0).all()
    assert dev <= bar, f"{tag}: distance {dev:.3e} over the bar {bar:.3e}"
    assert share <= 0.005, f"{tag}: {share:.4%} of the pixels beyond 1e-3 of the maximum"


CASES = {
    "far": dict(view="far"), "near": dict(view="near"), "pole": dict(view="pole"),
    "tilted": dict(view="far", kw=dict(disk_tilt=25.0)),
    "ragged": dict(view="far", W=61, H=43),
    "synthetic": dict(view="pole", catalog="synthetic"),
    "synthetic_far": dict(view="far", catalog="synthetic"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_plane_against_the_reference(case, hip_lib):
    c = CASES[case]
    pos = VIEWS[c["view"]]
    r = _mk(c.get("W", 96), c.get("H", 64), **c.get("kw", {}))
    r.build_ray_map(list(pos), FOV)
    dirs, flux = _synthetic() if c.get("catalog") == "synthetic" else _procedural(r, pos)
    r.set_stars(dirs, flux)
    got = r.read_star_plane()
    info = r.stars_info()
    S64, S32 = _references(r, pos, dirs, flux)
    r.close()
    assert info["n"] == len(dirs) and info["images"] > 0
    _check_plane(got, S64, S32, case)


def test_counts_and_resources(hip_lib):
    """The gather's counts against the reference's on the same planes (a triangle or a star within rounding of a threshold may
    fall on either side: 1 % of slack, the float32 reference's own disagreement is printed), and no scratch."""
    pos = VIEWS["far"]
    r = _mk()
    r.build_ray_map(list(pos), FOV)
    dirs, flux = _procedural(r, pos)
    r.set_stars(dirs, flux)
    r.read_star_plane()
    info = r.stars_info()
    p = r.ray_map_passes()
    d, f = _as_device(dirs, flux)
    _, st = R.star_plane(p["status"], p["escape_dir"], K.pixel_rays(_cam_dict(r, pos)), d, f, details=True)
    res = [r.stars_resources(False), r.stars_resources(True)]
    r.close()
    print(f"device {info}; reference images {st['images']} capped {st['capped']} skipped_span {st['skipped_span']}; resources {res}")
    for k in ("images", "capped", "skipped_span"):
        assert abs(info[k] - st[k]) <= max(1, 0.01 * st[k]), (k, info[k], st[k])
    assert (info["bins_theta"], info["bins_phi"]) == (19, 38) and info["max_magnification"] == 32.0 and info["max_span_deg"] == 10.0
    for x in res:
        assert x["scratch_bytes"] == 0 and 0 < x["vgprs"] <= 128 and 0 < x["lds_bytes"] <= 65536


def test_tiny_frame_is_all_zero(hip_lib):
    """5 x 3 at fov 90: every triangle spans more than 10 degrees."""
    r = _mk(5, 3)
    r.build_ray_map(list(VIEWS["far"]), FOV)
    dirs, flux = _procedural(r, VIEWS["far"])
    r.set_stars(dirs, flux)
    S = r.read_star_plane()
    info = r.stars_info()
    r.render_from_ray_map_async(frame=1, skip_bloom=True)
    r.sync()
    r.close()
    assert S.shape == (3, 5, 3) and not S.any() and info["images"] == 0 and info["skipped_span"] > 0


def test_two_gathers_give_the_same_bytes(hip_lib):
    pos = VIEWS["near"]
    r = _mk()
    r.build_ray_map(list(pos), FOV)
    dirs, flux = _procedural(r, pos)
    r.set_stars(dirs, flux)
    a = r.read_star_plane()
    r.set_stars(dirs, flux)                  # the cached plane is dropped with the catalogue it belonged to
    b = r.read_star_plane()
    r.build_ray_map(list(pos), FOV)          # ... and with the map
    c = r.read_star_plane()
    r.close()
    assert a.any() and a.tobytes() == b.tobytes() == c.tobytes()


# ---------------------------------------------------------------------------------------------------- the frame
def _layers(r):
    from bhr_amd import _lib
    return r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK)


def test_the_frame_adds_the_plane_to_the_sky(hip_lib):
    """One slot per pixel, so that the double-crossing pixels are on the overflow list."""
    pos = VIEWS["far"]
    r = _mk(options={"raymap_slots": 1})
    r.build_ray_map(list(pos), FOV)
    over = r.ray_map_info()["overflow_pixels"]
    p = r.ray_map_passes()
    r.render_from_ray_map_async(frame=3, skip_bloom=True)
    bg0, disk0 = _layers(r)
    dirs, flux = _procedural(r, pos)
    flux = flux * 40.0                       # bright enough for BG above 1
    r.set_stars(dirs, flux)
    r.render_from_ray_map_async(frame=3, skip_bloom=True)
    bg1, disk1 = _layers(r)
    S = r.read_star_plane()
    r.set_stars(np.zeros((0, 3)), np.zeros((0, 3)))
    r.render_from_ray_map_async(frame=3, skip_bloom=True)
    bg2, disk2 = _layers(r)
    r.set_stars(dirs, flux)
    r.clear_stars()
    assert r.stars_info()["n"] == 0
    r.render_from_ray_map_async(frame=3, skip_bloom=True)
    bg3, disk3 = _layers(r)
    r.close()
    assert over > 0 and S.any() and bg1.max() > 1.0
    assert np.array_equal(disk1, disk0)                                          # DISK untouched
    dark = ~S.any(axis=-1)
    assert np.array_equal(bg1[dark], bg0[dark])
    on_list = p["crossings"] > 1
    assert on_list.sum() == over and np.array_equal(bg1[on_list], bg0[on_list])  # the fix kernel stores them: no star light
    clear = (p["crossings"] == 0) & ~on_list
    assert (S[clear] > 0).any() and np.array_equal(bg1[clear], bg0[clear] + S[clear])      # fl(BG_without + S): one f32 addition
    rest = ~clear & ~on_list
    lo, hi = bg0[rest], (bg0[rest].astype(np.float64) + S[rest]).astype(np.float32)
    assert np.all(bg1[rest] >= np.nextafter(lo, np.float32(-1))) and np.all(bg1[rest] <= np.nextafter(hi, np.float32(np.inf)))
    for bg, disk in ((bg2, disk2), (bg3, disk3)):
        assert np.array_equal(bg, bg0) and np.array_equal(disk, disk0)


# ---------------------------------------------------------------------------------------------------- turned views
def _orbit(k, n=512, pov=VIEWS["far"]):
    from bhr_amd.camera import orbit_position
    return [float(v) for v in orbit_position(list(pov), k, n)]


def _frame(r):
    from bhr_amd import _lib
    return {k: r.read_layer(v) for k, v in (("final", _lib.LAYER_FINAL), ("bg", _lib.LAYER_BG), ("disk", _lib.LAYER_DISK))}


def test_angle_zero_is_the_map_frame(hip_lib):
    pos = VIEWS["far"]
    r = _mk()
    r.build_ray_map(_orbit(0), FOV)
    r.set_stars(*_procedural(r, pos))
    r.render_from_ray_map_async(frame=2)
    want = _frame(r)
    r.render_from_ray_map_async(frame=2, cam_pos=_orbit(0), fov=FOV)
    got = _frame(r)
    r.render_from_ray_map_async(frame=2, cam_pos=_orbit(37), fov=FOV)
    turned = _frame(r)
    r.close()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert (turned["bg"] != want["bg"]).any()


@pytest.mark.parametrize("k", [53, 256])
def test_turned_plane_is_the_build_plane_under_the_catalogue_turned_back(k, hip_lib):
    """Orbit positions 53 and 256 of 512: 37.27 and 180 degrees.  The plane of the view turned by the angle equals the build
    view's plane under the catalogue turned by the opposite angle (on the host, in binary64), to the bar above.  The turned
    view's plane is read out of its frame: under a BLACK sky BG is the plane itself on the pixels without a crossing; the
    others (the disk in front: BG = S (1 - alpha)) are left out of the comparison by giving them the reference's value."""
    from bhr_amd import _lib
    pos = VIEWS["far"]
    r = _mk()
    sky = np.zeros_like(_scene()[0])
    _lib.check(r._lib.bhr_set_skybox(r._ctx, _lib.fptr(sky), sky.shape[0], sky.shape[1]))
    r.build_ray_map(_orbit(0), FOV)
    p = r.ray_map_passes()
    dirs, flux = _procedural(r, pos)
    r.set_stars(dirs, flux)
    r.render_from_ray_map_async(frame=0, cam_pos=_orbit(k), fov=FOV, skip_bloom=True)
    bg = r.read_layer(_lib.LAYER_BG)
    angle = 2 * np.pi * k / 512
    S64, S32 = _references(r, _orbit(0), dirs, flux, angle=-angle)
    r.close()
    clear = (p["crossings"] == 0)
    got = np.where(clear[..., None], bg, S64.astype(np.float32))       # under a black sky BG = S where nothing is in front
    assert bg[clear].any()
    _check_plane(got, S64, S32, f"turned by {np.degrees(angle):.2f} degrees")


def test_four_frames_in_flight_on_two_slots(tmp_path, hip_lib):
    """Four frames queued without a sync, alternating two angles, each handed to a frame sink as it is queued: the files decode to
    the 8-bit rows of the same calls made one at a time.  The two frames in flight gather into the planes of their own slots."""
    from PIL import Image
    from bhr_amd.output import FrameSink
    pos = VIEWS["far"]
    r = _mk(frame_slots=2)
    r.build_ray_map(_orbit(0), FOV)
    dirs, flux = _procedural(r, pos)
    r.set_stars(dirs, flux * 20.0)
    ks = [41, 200, 41, 200]
    alone = []
    for j, k in enumerate(ks):
        r.render_from_ray_map_async(frame=j, cam_pos=_orbit(k), fov=FOV)
        alone.append(r.read_final_u8())                  # the read-back joins the frame
    with FrameSink(r, slots=4, workers=2) as sink:
        for j, k in enumerate(ks):
            r.render_from_ray_map_async(frame=j, cam_pos=_orbit(k), fov=FOV)
            sink.submit(str(tmp_path / f"f{j}.png"))
        frames, _ = sink.drain()
    r.close()
    assert frames == 4 and (alone[0] != alone[1]).any() and (alone[0] != alone[2]).any()
    for j in range(4):
        got = np.array(Image.open(tmp_path / f"f{j}.png").convert("RGB"))
        assert np.array_equal(got, alone[j]), j


# ---------------------------------------------------------------------------------------------------- behind the frame
def test_graded_frame_with_bg_above_one(hip_lib):
    """A frame graded with keep_hdr whose BG exceeds 1 is bhr_bloom + bhr_grade_frame run on the same BG and DISK."""
    from bhr_amd import _lib
    pos = VIEWS["far"]
    r = _mk()
    r.build_ray_map(list(pos), FOV)
    dirs, flux = _procedural(r, pos)
    r.set_stars(dirs, flux * 40.0)
    r.set_grade("reinhard", exposure=-0.5, transfer="srgb", keep_hdr=True)
    r.render_from_ray_map_async(frame=3)
    got = dict(final=r.read_layer(_lib.LAYER_FINAL), hdr=r.read_hdr(), blur=r.read_layer(_lib.LAYER_BLUR), u8=r.read_final_u8())
    bg, disk = _layers(r)
    r.clear_stars()
    r.render_from_ray_map_async(frame=3)
    plain = r.read_layer(_lib.LAYER_FINAL)
    r.write_layer(_lib.LAYER_BG, bg)
    r.write_layer(_lib.LAYER_DISK, disk)
    r.bloom_only()
    r.grade_frame()
    want = dict(final=r.read_layer(_lib.LAYER_FINAL), hdr=r.read_hdr(), blur=r.read_layer(_lib.LAYER_BLUR), u8=r.read_final_u8())
    r.close()
    assert bg.max() > 1.0 and got["hdr"].max() > 1.0 and got["final"].max() <= 1.0 and (got["final"] != plain).any()
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def _driver_scene(W, H, n_stars=400):
    return dict(width=W, height=H, cam_pos=[6.0, 0.0, 0.5], fov=90.0, step_size=0.1, n_stars=n_stars, tex_w=256, tex_h=128, math="fast")


def test_still_with_point_stars_is_the_map_frame(tmp_path, capsys, hip_lib):
    """drivers.render_image(stars=...) -- what --stars point runs for a still -- against the same calls made one at a time; the
    file decodes to its quantised frame.  (The BG and DISK layers are the strict arithmetic's whatever ``math`` says; the bloom
    follows it, as behind every frame from a map.)"""
    from PIL import Image
    from bhr_amd import _lib, drivers, skybox, stars
    sc = _driver_scene(64, 36)
    img = drivers.render_image(**sc, stars={"gain": 30.0})
    assert "Point stars: 400 stars" in capsys.readouterr().out
    drivers.save_image(img, str(tmp_path / "still.png"))
    file = np.array(Image.open(tmp_path / "still.png").convert("RGB"))
    baked = drivers.render_image(**sc)
    # one at a time
    r, use_lifecycle, n_r, n_phi = drivers.make_renderer(sc["width"], sc["height"], sc["cam_pos"], sc["fov"], n_stars=400, tex_w=256, tex_h=128, math="fast")
    assert use_lifecycle
    t = skybox.sky_tables(256, 128, 42, 400)
    r.build_procedural_skybox(seed=42, n_stars=400, starless=True)
    sky = r.read_skybox()
    cam = r.camera_uniforms(sc["cam_pos"], sc["fov"], 0)
    r.set_stars(*stars.catalog_from_tables(t, 30.0, float(cam.pixel_width) * float(cam.pixel_height)), max_magnification=32.0)
    factories = drivers.init_lifecycle_system(r, n_r, n_phi, seed=42)
    drivers.advance_lifecycle_frame(r, factories, t=0.0, dt=0.0, recompute_stats=True)
    r.build_ray_map(sc["cam_pos"], sc["fov"])
    r.render_from_ray_map_async(frame=0)
    want, want_u8 = r.read_layer(_lib.LAYER_FINAL), r.read_final_u8()
    S = r.read_star_plane()
    r.close()
    assert np.array_equal(img, want) and np.array_equal(file, want_u8)
    assert S.any() and (img != baked).any()
    # the starless sky is the procedural sky without the blobs: never brighter, and darker where a blob was
    full = skybox.generate_skybox(256, 128, 42, 400)
    assert (sky <= full + 1e-6).all() and (sky < full - 1e-3).any()


def test_orbit_map_video_with_point_stars(tmp_path, hip_lib):
    """Four 64 x 36 frames of an --orbit_map video with point stars: the files decode to the frames of the same calls made one
    at a time."""
    import os
    from PIL import Image
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    W, H, N, cam0, fov, speed = 64, 36, 4, [6.0, 0.0, 0.5], 90.0, 0.1
    st = {"gain": 30.0, "max_magnification": 32.0}

    def mk():
        return drivers.make_renderer(W, H, cam0, fov, n_stars=400, tex_w=256, tex_h=128, math="strict", stars=st)

    r, _, n_r, n_phi = mk()
    out = str(tmp_path / "v" / "v.mp4")
    try:
        drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=fov, static_cam_pos=cam0, orbit=True, orbit_degrees=90.0,
                             disk_rotation_speed=speed, video_stream="off", assemble=False, orbit_map=True, stars=st)
        with pytest.raises(ValueError, match="ray_map or orbit_map"):
            drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=str(tmp_path / "w" / "v.mp4"), fov=fov, static_cam_pos=cam0,
                                 orbit=True, video_stream="off", assemble=False, stars=st)
    finally:
        r.close()
    d = drivers._frames_dir(out)
    import json
    assert json.load(open(os.path.join(d, "progress.json")))["params"]["stars"] == st
    r, _, n_r, n_phi = mk()
    factories = drivers.init_lifecycle_system(r, n_r, n_phi, seed=42)
    r.build_ray_map(orbit_position(cam0, 0, N, 90.0), fov)
    frames = []
    for f in range(N):
        drivers.advance_lifecycle_frame(r, factories, f * speed, speed, recompute_stats=(f % 60 == 0))
        r.render_from_ray_map_async(frame=0, cam_pos=orbit_position(cam0, f, N, 90.0), fov=fov)
        frames.append(r.read_final_u8())
    lit = r.stars_info()["images"]
    r.close()
    assert lit > 0 and (frames[0] != frames[1]).any()
    for f in range(N):
        got = np.array(Image.open(os.path.join(d, f"frame_{f:04d}.png")).convert("RGB"))
        assert np.array_equal(got, frames[f]), f


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_rendering(hip_lib):
    import ctypes as C
    from bhr_amd import _lib
    pos = VIEWS["far"]
    r = _mk()
    r.build_ray_map(_orbit(0), FOV)
    dirs, flux = _procedural(r, pos)
    r.set_stars(dirs, flux)
    r.render_from_ray_map_async(frame=1)
    want = _frame(r)
    S = r.read_star_plane()
    rec = np.ascontiguousarray(np.concatenate(_as_device(dirs, flux), axis=1)[:8])

    def call(stars, n, par):
        return r._lib.bhr_set_stars(r._ctx, stars, n, par)

    def bad(mutate=None, n=8, par=None):
        a = rec.copy()
        if mutate:
            mutate(a)
        rc = call(a.ctypes.data, n, C.byref(_lib.StarParams(*par)) if par else None)
        assert rc == _lib.BHR_ERR_INVALID, (rc, r._lib.bhr_last_error())
        return r._lib.bhr_last_error().decode()

    assert r._lib.bhr_set_stars(None, rec.ctypes.data, 8, None) == _lib.BHR_ERR_INVALID
    assert "stars" in bad(n=-1) and "stars" in bad(n=(1 << 22) + 1)
    assert "unit vector" in bad(lambda a: a.__setitem__((3, 0), np.nan))
    assert "unit vector" in bad(lambda a: a.__setitem__((3, slice(0, 3)), a[3, :3] * 1.002))
    assert "flux" in bad(lambda a: a.__setitem__((2, 4), -1e-9)) and "flux" in bad(lambda a: a.__setitem__((2, 5), np.inf))
    assert "max_magnification" in bad(par=(0.5, 10.0)) and "max_magnification" in bad(par=(2e6, 10.0))
    assert "max_span_deg" in bad(par=(32.0, 0.0)) and "max_span_deg" in bad(par=(32.0, 61.0)) and "max_span_deg" in bad(par=(32.0, np.nan))
    with pytest.raises(ValueError):
        r.set_stars(dirs[:4] * 1.01, flux[:4])
    # shutter frames from the map refuse the catalogue
    with pytest.raises(AssertionError, match="star catalogue"):
        r.render_shutter_from_ray_map_async([0.0, 0.1])
    assert r.stars_info()["n"] == len(dirs) and r.ray_map_info()["built"] == 1
    # plane 9 stays unknown; a wrong size is refused
    buf = np.empty((64, 96, 3), dtype=np.float32)
    assert r._lib.bhr_raymap_read(r._ctx, 9, buf.ctypes.data, buf.nbytes) == _lib.BHR_ERR_INVALID
    assert r._lib.bhr_raymap_read(r._ctx, _lib.RAYMAP_STARS, buf.ctypes.data, buf.nbytes - 4) == _lib.BHR_ERR_INVALID
    r.render_from_ray_map_async(frame=1)
    got = _frame(r)
    assert np.array_equal(r.read_star_plane(), S)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # a supersampled map: render and plane read refuse, map and catalogue kept
    r.build_ray_map(_orbit(0), FOV, supersample=2)
    for fn in (lambda: r.render_from_ray_map_async(frame=1), lambda: r.render_from_ray_map_async(frame=1, cam_pos=_orbit(9), fov=FOV), r.read_star_plane):
        with pytest.raises(AssertionError, match="supersampled"):
            fn()
    assert r.stars_info()["n"] == len(dirs) and r.ray_map_info()["supersample"] == 2
    r.build_ray_map(_orbit(0), FOV)
    r.render_from_ray_map_async(frame=1)
    got = _frame(r)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # without a catalogue, and without a map, the plane is refused with BHR_ERR_STATE
    r.clear_stars()
    with pytest.raises(AssertionError, match="catalogue"):
        r.read_star_plane()
    r.render_shutter_from_ray_map_async([0.0, 0.1])      # ... and the shutter frame is back
    r.sync()
    r.set_stars(dirs, flux)
    r.free_ray_map()
    with pytest.raises(AssertionError, match="no ray map"):
        r.read_star_plane()
    r.close()
    # a row-block context has no catalogue
    rb = _mk(rows=(0, 32))
    with pytest.raises(ValueError, match="whole-frame"):
        rb.set_stars(dirs, flux)
    rb.close()
