"""Kerr point stars on the device (bhr_set_kerr_stars; include/bhr.h "Kerr point stars"): the star plane gathered
over the KERR ray map's planes against the brute-force binary64 reference (tests/stars_ref.py) fed the DEVICE's own STATUS and
ESCAPE_DIR planes, its repeatability, the frame that adds the plane to the sky under both redshifts, turned views, the
independence of the two catalogues and of the Kerr polarisation, the refusals, the resources and the drivers.

The bar of a plane is tests/test_gpu_stars.py's: four times the float32 reference's own distance from the binary64 one on the
same inputs, computed here, and at least 1e-6 (distances are shares of the plane's maximum: stars_ref.distance); and at most
0.5 % of the pixels further than 1e-3 of the maximum from the reference (tests/test_kerr_stars_ref.py: the float32 reference alone
has none over Kerr planes).

Scenes: scenes.analytic_skybox() and scenes.noisy_disk(), fov 90, step 0.1.  Frames 96 x 64 (crosses the gather's 15-pixel blocks
and the shade's 8 x 8 tiles), 61 x 43 (one pixel past four blocks, ragged tiles), 31 x 17 (one pixel past two blocks, two rows past
one), 5 x 3 (every triangle over the span), 1 x 1 and 2 x 1 (no cell at all)."""
import functools
import json
import os

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


def _mk(A=0.9, redshift="model", force=False, W=96, H=64, **kw):
    from bhr_amd import HipRenderer
    sky, tex = _scene()
    r = HipRenderer(W, H, sky, tex, math="strict", step_size=0.1, disk_tilt=0.0, anti_alias="disabled", **kw)
    if A != 0.0 or force:
        r.set_spin(A, force_kerr=force)
    if redshift == "exact":
        r.set_redshift("exact")
    return r


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
    """tests/test_gpu_stars.py's: poles, the phi = 0 seam from both sides, duplicates, and 3000 stars over the whole sphere."""
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


def _references(r, pos, dirs, flux, angle=0.0, passes=None, **kw):
    """(S64, S32): the binary64 and the float32 reference planes on the device's own KERR map planes; `angle`: the catalogue
    turned about z on the host in binary64 (a view turned by -angle)."""
    p = r.kerr_ray_map_passes() if passes is None else passes
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
    "far_prograde_model": dict(view="far", A=0.9),
    "far_retrograde_exact": dict(view="far", A=-0.9, redshift="exact"),
    "near_extreme": dict(view="near", A=0.998),
    "pole": dict(view="pole", A=0.9),
    "forced_spin_zero": dict(view="far", A=0.0, force=True),
    "ragged_61x43": dict(view="far", A=0.9, W=61, H=43),
    "ragged_31x17": dict(view="near", A=0.6, W=31, H=17),
    "synthetic_pole": dict(view="pole", A=0.9, catalog="synthetic"),
    "synthetic_far": dict(view="far", A=0.9, catalog="synthetic"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_plane_against_the_reference(case, hip_lib):
    c = CASES[case]
    pos = VIEWS[c["view"]]
    r = _mk(c["A"], c.get("redshift", "model"), c.get("force", False), c.get("W", 96), c.get("H", 64))
    r.build_kerr_ray_map(list(pos), FOV)
    dirs, flux = _synthetic() if c.get("catalog") == "synthetic" else _procedural(r, pos)
    r.set_kerr_stars(dirs, flux)
    got = r.read_kerr_star_plane()
    info = r.kerr_stars_info()
    S64, S32 = _references(r, pos, dirs, flux)
    r.close()
    assert info["n"] == len(dirs) and info["images"] > 0
    _check_plane(got, S64, S32, case)


def test_counts_and_resources(hip_lib):
    """The gather's counts over the Kerr map against the reference's on the same planes (a triangle or a star within rounding of
    a threshold may fall on either side: 1 % of slack), and no scratch in the four STARS shade kernels."""
    pos = VIEWS["far"]
    r = _mk(0.9)
    r.build_kerr_ray_map(list(pos), FOV)
    dirs, flux = _procedural(r, pos)
    r.set_kerr_stars(dirs, flux)
    r.read_kerr_star_plane()
    info = r.kerr_stars_info()
    p = r.kerr_ray_map_passes()
    d, f = _as_device(dirs, flux)
    _, st = R.star_plane(p["status"], p["escape_dir"], K.pixel_rays(_cam_dict(r, pos)), d, f, details=True)
    res = {(m, t): r.kerr_stars_resources(m, t) for m in ("model", "exact") for t in (False, True)}
    with pytest.raises(ValueError):
        r.kerr_stars_resources("fast")
    r.close()
    print(f"device {info}; reference images {st['images']} capped {st['capped']} skipped_span {st['skipped_span']}; resources {res}")
    for k in ("images", "capped", "skipped_span"):
        assert abs(info[k] - st[k]) <= max(1, 0.01 * st[k]), (k, info[k], st[k])
    assert (info["bins_theta"], info["bins_phi"]) == (19, 38) and info["max_magnification"] == 32.0 and info["max_span_deg"] == 10.0
    for x in res.values():
        assert x["scratch_bytes"] == 0 and x["lds_bytes"] == 0 and 0 < x["vgprs"] <= 128, res


def test_tiny_frame_is_all_zero(hip_lib):
    """5 x 3 at fov 90: every triangle spans more than 10 degrees."""
    r = _mk(0.9, W=5, H=3)
    r.build_kerr_ray_map(list(VIEWS["far"]), FOV)
    dirs, flux = _procedural(r, VIEWS["far"])
    r.set_kerr_stars(dirs, flux)
    S = r.read_kerr_star_plane()
    info = r.kerr_stars_info()
    r.render_from_kerr_ray_map_async(frame=1, skip_bloom=True)
    r.sync()
    r.close()
    assert S.shape == (3, 5, 3) and not S.any() and info["images"] == 0 and info["skipped_span"] > 0


def _frame(r):
    from bhr_amd import _lib
    return {k: r.read_layer(v) for k, v in (("final", _lib.LAYER_FINAL), ("bg", _lib.LAYER_BG), ("disk", _lib.LAYER_DISK))}


@pytest.mark.parametrize("size", [(1, 1), (2, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_without_a_cell(size, hip_lib):
    """No cell at all: the plane is zero and the frame is the frame without a catalogue, bit for bit."""
    W, H = size
    r = _mk(0.9, W=W, H=H)
    r.build_kerr_ray_map(list(VIEWS["far"]), FOV)
    r.render_from_kerr_ray_map_async(frame=1)
    want = _frame(r)
    dirs, flux = _procedural(r, VIEWS["far"])
    r.set_kerr_stars(dirs, flux)
    S = r.read_kerr_star_plane()
    info = r.kerr_stars_info()
    r.render_from_kerr_ray_map_async(frame=1)
    got = _frame(r)
    r.close()
    assert S.shape == (H, W, 3) and not S.any() and info["n"] == len(dirs) and info["images"] == 0
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_two_gathers_give_the_same_bytes(hip_lib):
    pos = VIEWS["near"]
    r = _mk(0.9)
    r.build_kerr_ray_map(list(pos), FOV)
    dirs, flux = _procedural(r, pos)
    r.set_kerr_stars(dirs, flux)
    a = r.read_kerr_star_plane()
    r.set_kerr_stars(dirs, flux)             # the cached plane is dropped with the catalogue it belonged to
    b = r.read_kerr_star_plane()
    r.build_kerr_ray_map(list(pos), FOV)     # ... and with the map
    c = r.read_kerr_star_plane()
    r.free_kerr_ray_map()                    # ... and a free drops it too: the plane of the next map is gathered anew
    r.build_kerr_ray_map(list(VIEWS["far"]), FOV)
    d = r.read_kerr_star_plane()
    r.close()
    assert a.any() and a.tobytes() == b.tobytes() == c.tobytes() and d.tobytes() != a.tobytes()


# ---------------------------------------------------------------------------------------------------- the frame
def _layers(r):
    from bhr_amd import _lib
    return r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK)


@pytest.mark.parametrize("redshift", ["model", "exact"])
def test_the_frame_adds_the_plane_to_the_sky(redshift, hip_lib):
    """One slot per pixel, so that the double-crossing pixels are on the overflow list."""
    pos = VIEWS["far"]
    r = _mk(0.9, redshift, options={"raymap_slots": 1})
    r.build_kerr_ray_map(list(pos), FOV)
    over = r.kerr_ray_map_info()["overflow_pixels"]
    p = r.kerr_ray_map_passes()
    r.render_from_kerr_ray_map_async(frame=3)
    bg0, disk0 = _layers(r)
    final0 = _frame(r)["final"]
    dirs, flux = _procedural(r, pos)
    flux = flux * 40.0                       # bright enough for BG above 1
    r.set_kerr_stars(dirs, flux)
    r.render_from_kerr_ray_map_async(frame=3)
    bg1, disk1 = _layers(r)
    S = r.read_kerr_star_plane()
    plain = []
    r.set_kerr_stars(dirs, np.zeros_like(flux))                     # a catalogue of zero fluxes
    r.render_from_kerr_ray_map_async(frame=3)
    plain.append(_frame(r))
    r.set_kerr_stars(np.zeros((0, 3)), np.zeros((0, 3)))            # n = 0
    assert r.kerr_stars_info()["n"] == 0
    r.render_from_kerr_ray_map_async(frame=3)
    plain.append(_frame(r))
    r.set_kerr_stars(dirs, flux)
    r.clear_kerr_stars()
    assert r.kerr_stars_info()["n"] == 0
    r.render_from_kerr_ray_map_async(frame=3)
    plain.append(_frame(r))
    r.close()
    assert over > 0 and S.any() and bg1.max() > 1.0
    assert np.array_equal(disk1, disk0)                                          # DISK untouched
    dark = ~S.any(axis=-1)
    assert dark.any() and np.array_equal(bg1[dark], bg0[dark])
    on_list = p["crossings"] > 1
    assert on_list.sum() == over and np.array_equal(bg1[on_list], bg0[on_list])  # the fix kernel stores them: no star light
    assert S[on_list].any()                                                      # ... although their plane values are not zero
    clear = (p["crossings"] == 0) & (p["status"] == 1)
    assert (S[clear] > 0).any() and np.array_equal(bg1[clear], bg0[clear] + S[clear])      # fl(BG_without + S): one f32 addition
    rest = ~clear & ~on_list
    lo, hi = bg0[rest], (bg0[rest].astype(np.float64) + S[rest]).astype(np.float32)
    assert np.all(bg1[rest] >= np.nextafter(lo, np.float32(-1))) and np.all(bg1[rest] <= np.nextafter(hi, np.float32(np.inf)))
    for n, f in enumerate(plain):
        assert f["bg"].tobytes() == bg0.tobytes() and f["disk"].tobytes() == disk0.tobytes() and f["final"].tobytes() == final0.tobytes(), n


# ---------------------------------------------------------------------------------------------------- turned views
def _orbit(k, n=512, pov=VIEWS["far"]):
    from bhr_amd.camera import orbit_position
    return [float(v) for v in orbit_position(list(pov), k, n)]


def test_angle_zero_is_the_map_frame(hip_lib):
    pos = VIEWS["far"]
    r = _mk(0.9)
    r.build_kerr_ray_map(_orbit(0), FOV)
    r.set_kerr_stars(*_procedural(r, pos))
    r.render_from_kerr_ray_map_async(frame=2)
    want = _frame(r)
    r.render_from_kerr_ray_map_async(frame=2, cam_pos=_orbit(0))
    got = _frame(r)
    r.render_from_kerr_ray_map_async(frame=2, cam_pos=_orbit(37))
    turned = _frame(r)
    r.close()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert (turned["bg"] != want["bg"]).any()


@pytest.mark.parametrize("k", [53, 256])
def test_turned_plane_is_the_build_plane_under_the_catalogue_turned_back(k, hip_lib):
    """Orbit positions 53 and 256 of 512: 37.27 and 180 degrees.  The plane of the view turned by the angle equals the build
    view's plane under the catalogue turned by the opposite angle (on the host, in binary64), to the bar above.  The turned
    view's plane is read out of its frame: under a BLACK sky BG is the plane itself on the pixels without a crossing; the
    others (the disk in front: BG = S (1 - alpha)) are left out of the comparison by giving them the reference's value."""
    from bhr_amd import _lib
    pos = VIEWS["far"]
    r = _mk(0.9)
    sky = np.zeros_like(_scene()[0])
    _lib.check(r._lib.bhr_set_skybox(r._ctx, _lib.fptr(sky), sky.shape[0], sky.shape[1]))
    r.build_kerr_ray_map(_orbit(0), FOV)
    p = r.kerr_ray_map_passes()
    dirs, flux = _procedural(r, pos)
    r.set_kerr_stars(dirs, flux)
    r.render_from_kerr_ray_map_async(frame=0, cam_pos=_orbit(k), skip_bloom=True)
    bg = r.read_layer(_lib.LAYER_BG)
    angle = 2 * np.pi * k / 512
    S64, S32 = _references(r, _orbit(0), dirs, flux, angle=-angle, passes=p)
    r.close()
    clear = (p["crossings"] == 0)
    got = np.where(clear[..., None], bg, S64.astype(np.float32))       # under a black sky BG = S where nothing is in front
    assert bg[clear].any()
    _check_plane(got, S64, S32, f"turned by {np.degrees(angle):.2f} degrees")


def test_four_frames_in_flight_on_two_slots(tmp_path, hip_lib):
    """Four frames with four different turns queued without a sync, each handed to a frame sink as it is queued: the files decode
    to the 8-bit rows of the same calls made one at a time.  The two frames in flight gather into the planes of their own slots."""
    from PIL import Image
    from bhr_amd.output import FrameSink
    pos = VIEWS["far"]
    r = _mk(0.9, frame_slots=2)
    r.build_kerr_ray_map(_orbit(0), FOV)
    dirs, flux = _procedural(r, pos)
    r.set_kerr_stars(dirs, flux * 20.0)
    ks = [41, 200, 77, 300]
    alone = []
    for j, k in enumerate(ks):
        r.render_from_kerr_ray_map_async(frame=j, cam_pos=_orbit(k))
        alone.append(r.read_final_u8())                  # the read-back joins the frame
    with FrameSink(r, slots=4, workers=2) as sink:
        for j, k in enumerate(ks):
            r.render_from_kerr_ray_map_async(frame=j, cam_pos=_orbit(k))
            sink.submit(str(tmp_path / f"f{j}.png"))
        frames, _ = sink.drain()
    r.close()
    assert frames == 4 and (alone[0] != alone[1]).any() and (alone[0] != alone[2]).any()
    for j in range(4):
        got = np.array(Image.open(tmp_path / f"f{j}.png").convert("RGB"))
        assert np.array_equal(got, alone[j]), j


# ---------------------------------------------------------------------------------------------------- independence
def test_the_schwarzschild_catalogue_leaves_the_kerr_frame_alone(hip_lib):
    pos = VIEWS["far"]
    r = _mk(0.9)
    r.build_kerr_ray_map(_orbit(0), FOV)
    r.render_from_kerr_ray_map_async(frame=1)
    want = _frame(r)
    r.render_from_kerr_ray_map_async(frame=1, cam_pos=_orbit(19))
    want_turned = _frame(r)
    dirs, flux = _procedural(r, pos)
    r.set_stars(dirs, flux * 40.0)
    assert r.stars_info()["n"] == len(dirs) and r.kerr_stars_info()["n"] == 0
    r.render_from_kerr_ray_map_async(frame=1)
    got = _frame(r)
    r.render_from_kerr_ray_map_async(frame=1, cam_pos=_orbit(19))
    got_turned = _frame(r)
    r.render_shutter_from_kerr_ray_map_async([0.0, 0.1])             # the shutter frame does not ask about it either
    r.sync()
    with pytest.raises(AssertionError, match="bhr_set_kerr_stars"):
        r.read_kerr_star_plane()                                     # no KERR catalogue
    r.close()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes() and got_turned[k].tobytes() == want_turned[k].tobytes(), k


def test_the_kerr_catalogue_leaves_the_schwarzschild_frame_alone(hip_lib):
    pos = VIEWS["far"]
    r = _mk(0.0)
    r.build_ray_map(_orbit(0), FOV)
    r.render_from_ray_map_async(frame=1)
    want = _frame(r)
    dirs, flux = _procedural(r, pos)
    r.set_kerr_stars(dirs, flux * 40.0)                              # needs no spin
    assert r.kerr_stars_info()["n"] == len(dirs) and r.stars_info()["n"] == 0
    r.render_from_ray_map_async(frame=1)
    got = _frame(r)
    r.render_shutter_from_ray_map_async([0.0, 0.1])                  # not refused: that is bhr_set_stars' catalogue's
    r.sync()
    with pytest.raises(AssertionError, match="catalogue"):
        r.read_star_plane()
    # both set: each map shows its own
    r.set_stars(dirs[:200], flux[:200] * 40.0)
    S = r.read_star_plane()
    r.render_from_ray_map_async(frame=1, skip_bloom=True)
    bg = _layers(r)[0]
    r.clear_kerr_stars()
    r.render_from_ray_map_async(frame=1, skip_bloom=True)
    bg_again = _layers(r)[0]
    r.close()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert S.any() and (bg != want["bg"]).any() and bg.tobytes() == bg_again.tobytes()


@pytest.mark.parametrize("redshift", ["model", "exact"])
def test_the_stokes_planes_do_not_depend_on_the_catalogue(redshift, hip_lib):
    pos = VIEWS["far"]
    r = _mk(0.9, redshift)
    r.set_kerr_polarization("toroidal", 0.7, 16)
    r.build_kerr_ray_map(list(pos), FOV)
    r.render_from_kerr_ray_map_async(frame=2)
    want, planes, cells = _frame(r), r.stokes(), r.stokes_cells()
    dirs, flux = _procedural(r, pos)
    r.set_kerr_stars(dirs, flux * 40.0)
    r.render_from_kerr_ray_map_async(frame=2)
    got, planes1, cells1 = _frame(r), r.stokes(), r.stokes_cells()
    r.close()
    assert planes.any() and planes1.tobytes() == planes.tobytes() and cells1.tobytes() == cells.tobytes()
    assert got["disk"].tobytes() == want["disk"].tobytes() and (got["bg"] != want["bg"]).any()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_rendering(hip_lib):
    import ctypes as C
    from bhr_amd import _lib
    pos = VIEWS["far"]
    r = _mk(0.9)
    dirs, flux = _procedural(r, pos)
    buf = np.empty((64, 96, 3), dtype=np.float32)

    def state(call):
        rc = call()
        msg = r._lib.bhr_last_error().decode()
        assert rc == _lib.BHR_ERR_STATE, (rc, msg)
        return msg

    # without a map, with and without a catalogue
    assert "no Kerr ray map" in state(lambda: r._lib.bhr_kerr_raymap_read(r._ctx, _lib.RAYMAP_STARS, buf.ctypes.data, buf.nbytes))
    r.set_kerr_stars(dirs, flux)
    assert "no Kerr ray map" in state(lambda: r._lib.bhr_kerr_raymap_read(r._ctx, _lib.RAYMAP_STARS, buf.ctypes.data, buf.nbytes))
    r.build_kerr_ray_map(_orbit(0), FOV)
    r.render_from_kerr_ray_map_async(frame=1)
    want = _frame(r)
    S = r.read_kerr_star_plane()
    # the setter's own checks, in its own name
    rec = np.ascontiguousarray(np.concatenate(_as_device(dirs, flux), axis=1)[:8])
    assert r._lib.bhr_set_kerr_stars(None, rec.ctypes.data, 8, None) == _lib.BHR_ERR_INVALID
    for n, par, word in ((-1, None, "stars"), ((1 << 22) + 1, None, "stars"), (8, (0.5, 10.0), "max_magnification"), (8, (32.0, 61.0), "max_span_deg")):
        rc = r._lib.bhr_set_kerr_stars(r._ctx, rec.ctypes.data, n, C.byref(_lib.StarParams(*par)) if par else None)
        msg = r._lib.bhr_last_error().decode()
        assert rc == _lib.BHR_ERR_INVALID and "bhr_set_kerr_stars" in msg and word in msg, (rc, msg)
    bad = rec.copy()
    bad[3, 0] = np.nan
    assert r._lib.bhr_set_kerr_stars(r._ctx, bad.ctypes.data, 8, None) == _lib.BHR_ERR_INVALID and "unit vector" in r._lib.bhr_last_error().decode()
    # shutter frames from the map refuse the catalogue
    cams = (_lib.Camera * 2)()
    for j in range(2):
        cams[j] = r.camera_uniforms(_orbit(0), FOV, t_offset=0.1 * j)
    msg = state(lambda: r._lib.bhr_kerr_raymap_render_shutter(r._ctx, cams, 2, 0))
    assert "star" in msg and "bhr_set_kerr_stars" in msg
    # a wrong size of the plane is refused
    assert r._lib.bhr_kerr_raymap_read(r._ctx, _lib.RAYMAP_STARS, buf.ctypes.data, buf.nbytes - 4) == _lib.BHR_ERR_INVALID
    assert r.kerr_stars_info()["n"] == len(dirs) and r.kerr_ray_map_info()["built"] == 1
    r.render_from_kerr_ray_map_async(frame=1)
    got = _frame(r)
    assert r.read_kerr_star_plane().tobytes() == S.tobytes()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    # a supersampled Kerr map: render, view and plane read refuse, map and catalogue kept
    r.build_kerr_ray_map(_orbit(0), FOV, supersample=2)
    view = r.camera_uniforms(_orbit(9), FOV, 1)
    for call in (lambda: r._lib.bhr_kerr_raymap_render(r._ctx, 0.1, 0), lambda: r._lib.bhr_kerr_raymap_render_view(r._ctx, C.byref(view), 0),
                 lambda: r._lib.bhr_kerr_raymap_read(r._ctx, _lib.RAYMAP_STARS, buf.ctypes.data, buf.nbytes),
                 lambda: r._lib.bhr_kerr_raymap_render_shutter(r._ctx, cams, 2, 0)):
        msg = state(call)
        assert "star" in msg, msg
    assert r.kerr_stars_info()["n"] == len(dirs) and r.kerr_ray_map_info()["supersample"] == 2
    r.build_kerr_ray_map(_orbit(0), FOV)
    r.render_from_kerr_ray_map_async(frame=1)
    got = _frame(r)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    # without a catalogue the plane is refused, and the shutter frame and the supersampled map are back
    r.clear_kerr_stars()
    assert "bhr_set_kerr_stars" in state(lambda: r._lib.bhr_kerr_raymap_read(r._ctx, _lib.RAYMAP_STARS, buf.ctypes.data, buf.nbytes))
    r.render_shutter_from_kerr_ray_map_async([0.0, 0.1])
    r.sync()
    r.close()
    # a row-block context has no catalogue
    rb = _mk(0.0, rows=(0, 32))
    with pytest.raises(ValueError, match="whole-frame"):
        rb.set_kerr_stars(dirs, flux)
    rb.close()


# ---------------------------------------------------------------------------------------------------- the drivers
SC = dict(width=64, height=36, cam_pos=[6.0, 0.0, 0.5], fov=90.0, step_size=0.1, n_stars=400, tex_w=256, tex_h=128, math="strict")


def _one_at_a_time(gain=30.0):
    """The renderer drivers.render_image(kerr_stars=) makes, by the same calls made one at a time; -> (renderer, factories)."""
    from bhr_amd import drivers, skybox, stars
    r, use_lifecycle, n_r, n_phi = drivers.make_renderer(SC["width"], SC["height"], SC["cam_pos"], SC["fov"], n_stars=400, tex_w=256, tex_h=128,
                                                         math="strict", spin=0.9)
    assert use_lifecycle
    r.build_procedural_skybox(seed=42, n_stars=400, starless=True)
    cam = r.camera_uniforms(SC["cam_pos"], SC["fov"], 0)
    r.set_kerr_stars(*stars.catalog_from_tables(skybox.sky_tables(256, 128, 42, 400), gain, float(cam.pixel_width) * float(cam.pixel_height)),
                     max_magnification=32.0)
    return r, drivers.init_lifecycle_system(r, n_r, n_phi, seed=42)


def test_still_with_kerr_point_stars_and_its_passes(tmp_path, capsys, hip_lib):
    """drivers.render_image(kerr_stars=, kerr_passes_path=) -- what --spin_stars point --spin_passes runs for a still -- against the
    same calls made one at a time; the passes file holds the planes of kerr_ray_map_passes() and the frame's layers."""
    from bhr_amd import _lib, drivers
    path = str(tmp_path / "p" / "passes.npz")
    img = drivers.render_image(**SC, spin=0.9, kerr_stars={"gain": 30.0}, kerr_passes_path=path)
    out = capsys.readouterr().out
    assert "Kerr point stars: 400 stars" in out and "Saved: " + path in out
    baked = drivers.render_image(**SC, spin=0.9)
    r, factories = _one_at_a_time()
    drivers.advance_lifecycle_frame(r, factories, t=0.0, dt=0.0, recompute_stats=True)
    r.build_kerr_ray_map(SC["cam_pos"], SC["fov"])
    r.render_from_kerr_ray_map_async(frame=0)
    want = r.read_layer(_lib.LAYER_FINAL)
    layers = dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), blur=r.read_layer(_lib.LAYER_BLUR))
    passes = r.kerr_ray_map_passes()
    S = r.read_kerr_star_plane()
    r.close()
    assert img.tobytes() == want.tobytes() and S.any() and (img != baked).any()
    z = np.load(path)
    assert set(z.files) == set(passes) | set(layers) | {"spin", "redshift"}
    for k, v in {**passes, **layers}.items():
        assert z[k].dtype == v.dtype and z[k].tobytes() == v.tobytes(), k
    assert z["spin"] == np.float32(0.9) and str(z["redshift"]) == "model"


def test_passes_of_a_marched_still_under_a_spin(tmp_path, hip_lib):
    """--spin_passes alone: the image is the marched frame it is without the flag, the file holds the view's Kerr map."""
    from bhr_amd import drivers
    path = str(tmp_path / "passes.npz")
    plain = drivers.render_image(**SC, spin=-0.9, redshift="exact")
    img = drivers.render_image(**SC, spin=-0.9, redshift="exact", kerr_passes_path=path)
    z = np.load(path)
    assert img.tobytes() == plain.tobytes()
    assert z["status"].shape == (36, 64) and z["hits"].shape[1:] == (36, 64, 5) and z["bg"].shape == (36, 64, 3)
    assert z["spin"] == np.float32(-0.9) and str(z["redshift"]) == "exact" and (z["status"] == 1).any() and (z["crossings"] > 0).any()
    # the frame's layers are the marched frame's: final = clip(bg + disk + blur) is not re-derived here, the layers are not blank
    assert z["bg"].any() and z["disk"].any()


def test_spin_map_orbit_video_with_kerr_point_stars(tmp_path, hip_lib):
    """Four 64 x 36 frames of a --spin_map --orbit video with Kerr point stars: the files decode to the frames of the same calls
    made one at a time, each with the star plane of its own turned view."""
    from PIL import Image
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    W, H, N, cam0, fov, speed = 64, 36, 4, SC["cam_pos"], 90.0, 0.1
    st = {"gain": 30.0, "max_magnification": 32.0}
    r, _, n_r, n_phi = drivers.make_renderer(W, H, cam0, fov, n_stars=400, tex_w=256, tex_h=128, math="strict", spin=0.9, kerr_stars=st)
    out = str(tmp_path / "v" / "v.mp4")
    try:
        drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=fov, static_cam_pos=cam0, orbit=True, orbit_degrees=90.0,
                             disk_rotation_speed=speed, video_stream="off", assemble=False, spin_map=True, kerr_stars=st)
        with pytest.raises(ValueError, match="--spin_map"):
            drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=str(tmp_path / "w" / "v.mp4"), fov=fov, static_cam_pos=cam0,
                                 orbit=True, video_stream="off", assemble=False, kerr_stars=st)
    finally:
        r.close()
    d = drivers._frames_dir(out)
    params = json.load(open(os.path.join(d, "progress.json")))["params"]
    assert params["kerr_stars"] == st and params["spin_map"] is True and "stars" not in params
    r, factories = _one_at_a_time()
    r.build_kerr_ray_map(orbit_position(cam0, 0, N, 90.0), fov)
    frames = []
    for f in range(N):
        drivers.advance_lifecycle_frame(r, factories, f * speed, speed, recompute_stats=(f % 60 == 0))
        r.render_from_kerr_ray_map_async(frame=0, cam_pos=orbit_position(cam0, f, N, 90.0))
        frames.append(r.read_final_u8())
    lit = r.kerr_stars_info()["images"]
    r.close()
    assert lit > 0 and (frames[0] != frames[1]).any()
    for f in range(N):
        got = np.array(Image.open(os.path.join(d, f"frame_{f:04d}.png")).convert("RGB"))
        assert np.array_equal(got, frames[f]), f
