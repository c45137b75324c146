"""The ray map on the device (bhr_raymap_build / _render / _read; include/bhr.h states the contract): a frame shaded from the
map is bit for bit the strict bhr_render of the build's view under the scene as it is at the time of the call, whatever the
slot count; the map's planes are the strict march's own step counts, fates, escape directions and hit points.

The frames are the suite's small ones: 21 x 13 has partial tiles on both sides, 24 x 15 is tilted and anti-aliased (the records
carry the differentials), 96 x 54 has the hole's image and rays with several crossings."""
import ctypes as C
import functools
import io
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VIEWS = {
    "odd": dict(W=21, H=13, cam=(6.0, 0.0, 0.5), fov=90.0, kw=()),
    "tilt": dict(W=24, H=15, cam=(5.0, 2.0, 1.0), fov=80.0, kw=(("anti_alias", "lod_radius"), ("disk_tilt", 20.0))),
    "ring": dict(W=96, H=54, cam=(6.0, 0.0, 0.5), fov=90.0, kw=()),
}
LAYERS = ("final", "bg", "disk", "blur")
TS = (0.0, 0.3, 7.5)
R_INNER, R_OUTER = np.float32(2.0), np.float32(15.0)


@functools.lru_cache(maxsize=None)
def _scene(which):
    """"a": the scene the maps are built under; "b": the one they are rendered under (other sky, other texture seed)."""
    from bhr_amd import scenes
    return (scenes.analytic_skybox(), scenes.noisy_disk(seed=7)) if which == "a" else (scenes.star_skybox(), scenes.noisy_disk(seed=11))


def _mk(view, math_mode="strict", scene="a", **kw):
    from bhr_amd import HipRenderer
    v = VIEWS[view]
    sky, tex = _scene(scene)
    return HipRenderer(v["W"], v["H"], sky, tex, math=math_mode, **dict(v["kw"]), **kw)


def _set_scene(r, which):
    from bhr_amd import _lib
    sky, tex = _scene(which)
    _lib.check(r._lib.bhr_set_skybox(r._ctx, _lib.fptr(sky), sky.shape[0], sky.shape[1]))
    r.update_disk_texture(tex)


def _build(r, view, **kw):
    r.build_ray_map(list(VIEWS[view]["cam"]), VIEWS[view]["fov"], **kw)


def _render(r, view, t, flags=0):
    """bhr_render of the view with t_offset = t under the strict arithmetic."""
    from bhr_amd import _lib
    cam = r.camera_uniforms(list(VIEWS[view]["cam"]), VIEWS[view]["fov"], t_offset=t)
    _lib.check(r._lib.bhr_render(r._ctx, C.byref(cam), flags | _lib.FORCE_STRICT))


def _read(r, names=LAYERS):
    from bhr_amd import _lib
    ids = dict(final=_lib.LAYER_FINAL, bg=_lib.LAYER_BG, disk=_lib.LAYER_DISK, blur=_lib.LAYER_BLUR)
    out = {k: r.read_layer(ids[k]) for k in names}
    out["u8"] = r.read_final_u8()
    return out


@functools.lru_cache(maxsize=None)
def _rendered(view, scene, t, flags=0, math_mode="strict"):
    """The marched frame: computed once, shared by the tests, never modified."""
    r = _mk(view, math_mode, scene)
    _render(r, view, t, flags)
    out = _read(r)
    out["c"] = r.counters()
    r.close()
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _assert_equal(got, want, tag, names=LAYERS + ("u8",)):
    for k in names:
        bad = int((got[k] != want[k]).any(axis=-1).sum())
        assert bad == 0, f"{tag} {k}: {bad} pixels differ (max |d| {np.abs(got[k].astype(np.float64) - want[k]).max():.3g})"


# ---- 1. re-shade equals render ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", list(VIEWS))
def test_map_frame_is_the_strict_render_under_the_current_scene(view, hip_lib):
    r = _mk(view, scene="a")
    _build(r, view)
    _set_scene(r, "b")                                   # between build and render: the map does not hold the scene
    for t in TS:
        r.render_from_ray_map_async(t_offset=t)
        got = _read(r)
        _assert_equal(got, _rendered(view, "b", t), f"{view} t={t}")
        old = _rendered(view, "a", t)
        assert (got["bg"] != old["bg"]).any() and (got["disk"] != old["disk"]).any(), "the scene swap changed nothing: the test cannot fail"
    assert (_rendered(view, "b", 0.0)["disk"] != _rendered(view, "b", 7.5)["disk"]).any()      # t_offset matters
    c = r.counters()
    assert c["rays"] == VIEWS[view]["W"] * VIEWS[view]["H"]
    r.close()


@pytest.mark.parametrize("view", ["odd", "tilt"])
def test_map_without_differentials(view, hip_lib):
    from bhr_amd import _lib
    r = _mk(view, scene="a")
    _build(r, view, skip_differentials=True)
    assert r.ray_map_info()["diff"] == 0
    _set_scene(r, "b")
    r.render_from_ray_map_async(t_offset=0.3)
    got = _read(r)
    r.close()
    _assert_equal(got, _rendered(view, "b", 0.3, _lib.SKIP_DIFFERENTIALS), f"{view} skip_differentials")
    if view == "tilt":                                   # anti-aliased: the differentials change the picture
        assert (got["disk"] != _rendered(view, "b", 0.3)["disk"]).any()


@pytest.mark.parametrize("what", ["skip_bloom", "lens_flare"])
def test_map_frame_flags(what, hip_lib):
    from bhr_amd import _lib
    r = _mk("tilt", scene="a")
    _build(r, "tilt")
    assert r.ray_map_info()["diff"] == 1
    _set_scene(r, "b")
    r.render_from_ray_map_async(t_offset=0.3, skip_bloom=what == "skip_bloom", lens_flare=what == "lens_flare")
    got = _read(r)
    r.close()
    _assert_equal(got, _rendered("tilt", "b", 0.3, _lib.SKIP_BLOOM if what == "skip_bloom" else _lib.LENS_FLARE), what)
    assert (got["final"] != _rendered("tilt", "b", 0.3)["final"]).any()


# ---- 2. any slot count gives the same frame -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ring_map(slots):
    r = _mk("ring", scene="a", options={"raymap_slots": slots})
    _build(r, "ring")
    out = dict(info=r.ray_map_info(), passes=r.ray_map_passes())
    r.render_from_ray_map_async(t_offset=0.3)
    out["frame"] = _read(r)
    out["c"] = r.counters()
    r.close()
    return out


@pytest.mark.parametrize("slots", [1, 4, 8])
def test_any_slot_count_gives_the_same_frame(slots, hip_lib):
    m = _ring_map(slots)
    _assert_equal(m["frame"], _rendered("ring", "a", 0.3), f"K={slots}")
    p, info = m["passes"], m["info"]
    assert info["slots"] == slots and p["hits"].shape == (slots, 54, 96, 5)
    over = p["crossings"] > slots
    assert info["overflow_pixels"] == int(over.sum())
    assert info["crossings_stored"] == int(np.minimum(p["crossings"], slots).sum())
    # the frame's counters: the steps of the overflow re-march only
    assert m["c"]["ray_steps"] == int(p["steps"][over].sum())
    assert m["c"]["rays"] == 96 * 54 and m["c"]["frames_timed"] == 1
    assert m["c"]["march_ms"] > 0 and m["c"]["frame_ms"] >= m["c"]["march_ms"]
    if slots == 1:
        assert info["overflow_pixels"] > 0
    if slots == 8:
        assert info["overflow_pixels"] < _ring_map(1)["info"]["overflow_pixels"]
    assert info["device_bytes"] >= 96 * 54 * (24 + slots * 20)


# ---- 3. passes against the oracle's f32 build -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _map_of(view):
    r = _mk(view, scene="a")
    _build(r, view)
    out = dict(info=r.ray_map_info(), passes=r.ray_map_passes())
    r.render_from_ray_map_async(t_offset=0.0)
    out["frame"] = _read(r)
    r.close()
    return out


@pytest.mark.parametrize("view", list(VIEWS))
def test_passes_against_the_oracle(view, oracle, hip_lib):
    v = VIEWS[view]
    sky, tex = _scene("a")
    o = oracle.OracleRenderer(v["W"], v["H"], sky, tex, **dict(v["kw"]))
    o.march(list(v["cam"]), v["fov"])
    m = _map_of(view)
    p = m["passes"]
    np.testing.assert_array_equal(p["steps"], o.last_steps.T)
    assert int(p["steps"].sum()) == m["info"]["ray_steps"] == _rendered(view, "a", 0.0)["c"]["ray_steps"] == o.last_total_steps
    esc = o.escape_directions(list(v["cam"]), v["fov"]).transpose(1, 0, 2)
    np.testing.assert_array_equal(p["status"] == 1, (esc != 0).any(axis=-1))
    assert set(np.unique(p["status"])) <= {0, 1, 2} and (p["status"] == 1).any()
    if view == "ring":
        assert (p["status"] == 0).any()                  # the hole's image
    # bit-identical paths; only the three roundings of the normalisation can differ: 1e-6 is 16 ulp of 1
    err = np.abs(p["escape_dir"].astype(np.float64) - esc).max()
    print(f"{view}: max |escape_dir - oracle| = {err:.3g}")
    assert err <= 1e-6
    assert (p["escape_dir"][p["status"] != 1] == 0).all()


def test_steps_equal_the_reference_statements_fixture(hip_lib):
    from bhr_amd import HipRenderer
    from test_reference_kernels import KW, load_scene
    g, sky, tex = load_scene("default")
    r = HipRenderer(int(g["width"]), int(g["height"]), sky, tex, **KW["default"])
    r.build_ray_map(list(g["cam_pos"]), float(g["fov"]))
    steps = r.ray_map_passes()["steps"]
    r.close()
    ref = np.asarray(g["f32_steps"])
    assert ref.shape == steps.shape[::-1]                # the fixture keeps the reference's (W, H) field layout
    np.testing.assert_array_equal(steps, ref.T)


# ---- 4. hit records are self-consistent -----------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["tilt", "ring"])
def test_hit_records_are_self_consistent(view, hip_lib):
    from bhr_amd.output import hit_polar
    m = _map_of(view)
    p, K = m["passes"], m["info"]["slots"]
    hits, cr = p["hits"], p["crossings"]
    assert hits.shape[3] == (9 if view == "tilt" else 5) and hits.dtype == np.float32
    assert (cr > 0).any() and (cr == 0).any()
    assert (m["frame"]["disk"][cr == 0] == 0).all()
    stored = np.arange(K)[:, None, None] < np.minimum(cr, K)[None]
    hx, hy = hits[..., 0], hits[..., 1]
    rr = np.sqrt(hx * hx + hy * hy, dtype=np.float32)        # the kernel's operations in its order: two products, a sum, a root
    assert (rr[stored] >= R_INNER).all() and (rr[stored] <= R_OUTER).all()
    assert (hits[~stored] == 0).all()
    to_cam = hits[..., 2:5][stored]
    # minus the ray's direction at the start of the step: not a unit vector (the march never re-normalises d), never zero
    assert np.isfinite(to_cam).all() and (np.linalg.norm(to_cam.astype(np.float64), axis=-1) > 0.5).all()
    if view == "tilt":
        assert (hits[..., 5:][stored] != 0).any()
    hr, hphi = hit_polar(hits, cr)
    np.testing.assert_array_equal(hr, p["hit_r"])
    np.testing.assert_array_equal(hphi, p["hit_phi"])
    assert np.isnan(p["hit_r"][cr == 0]).all() and np.isnan(p["hit_phi"][cr == 0]).all()
    np.testing.assert_array_equal(p["hit_r"][cr > 0], rr[0][cr > 0])
    np.testing.assert_array_equal(p["hit_phi"][cr > 0], np.arctan2(hy[0], hx[0], dtype=np.float32)[cr > 0])


# ---- 5. other arithmetics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode,view", [("fast", "tilt"), ("hybrid", "ring")])
def test_maps_on_other_arithmetics_are_strict(math_mode, view, hip_lib):
    r = _mk(view, math_mode, scene="a")
    _build(r, view)
    r.render_from_ray_map_async(t_offset=0.3)
    got = _read(r)
    _render(r, view, 0.3)                                # BHR_FORCE_STRICT on the same context
    want = _read(r)
    r.render_async(list(VIEWS[view]["cam"]), VIEWS[view]["fov"])      # the context's own arithmetic still renders
    own = _read(r)
    r.close()
    _assert_equal(got, want, f"{math_mode} {view}")
    _assert_equal(got, _rendered(view, "a", 0.3), f"{math_mode} {view} vs a strict context")
    assert np.isfinite(own["final"]).all() and (own["final"] > 0).any()


# ---- 6. frame slots and consumers -----------------------------------------------------------------------------------------
def test_map_frames_interleaved_on_two_slots_equal_one_slot(hip_lib):
    view, fov = "ring", VIEWS["ring"]["fov"]

    def sequence(slots):
        r = _mk(view, "hybrid", scene="a", frame_slots=slots)
        assert r.frame_slots == slots
        _build(r, view)
        frames = []
        for step in ("map0", "plain", "map1", "plain2", "map0"):
            if step == "map0":
                r.render_from_ray_map_async(t_offset=0.0)
            elif step == "map1":
                r.render_from_ray_map_async(t_offset=7.5)
            elif step == "plain":
                r.render_async([3.2, 0.5, 0.12], 100.0)
            else:
                r.render_async(list(VIEWS[view]["cam"]), fov)
            frames.append(_read(r))
        r.close()
        return frames

    one, two = sequence(1), sequence(2)
    for k, (g, w) in enumerate(zip(two, one)):
        _assert_equal(g, w, f"frame {k}")
    _assert_equal(two[4], two[0], "map0 again")
    _assert_equal(two[0], _rendered(view, "a", 0.0), "map0")
    _assert_equal(two[2], _rendered(view, "a", 7.5), "map1")
    assert (two[0]["final"] != two[2]["final"]).any() and (two[0]["final"] != two[1]["final"]).any()


def test_device_png_and_jpeg_of_a_map_frame(hip_lib):
    from PIL import Image
    from bhr_amd import output
    files = {}
    for how in ("map", "march"):
        r = _mk("ring", scene="a")
        if how == "map":
            _build(r, "ring")
            r.render_from_ray_map_async(t_offset=0.3)
        else:
            _render(r, "ring", 0.3)
        files[how] = (output.png_encode_device(r), output.jpeg_encode_device(r, 90), r.read_final_u8())
        r.close()
    png, jpg, u8 = files["map"]
    np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), u8)
    # JPEG is lossy: "decodes to the rows" is that the file is the baseline JPEG of exactly those rows (tests/jpeg_ref.py)
    import jpeg_ref
    assert jpg == jpeg_ref.encode(u8, 90, output.jpeg_restart_interval(u8.shape[1]))
    assert np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB")).shape == u8.shape
    assert png == files["march"][0] and jpg == files["march"][1]
    np.testing.assert_array_equal(u8, files["march"][2])


@pytest.mark.parametrize("what", ["grade", "dither"])
def test_graded_and_dithered_map_frames(what, hip_lib):
    got = {}
    for how in ("map", "march"):
        r = _mk("tilt", scene="a")
        if what == "grade":
            r.set_grade("aces", exposure=0.5, transfer="srgb", keep_hdr=True)
        else:
            r.set_dither("blue")
        if how == "map":
            _build(r, "tilt")
            r.render_from_ray_map_async(t_offset=0.3)
        else:
            _render(r, "tilt", 0.3)
        got[how] = _read(r)
        got[how]["u16"] = r.read_final_u16()
        if what == "grade":
            got[how]["hdr"] = r.read_hdr()
        r.close()
    _assert_equal(got["map"], got["march"], what, LAYERS + ("u8", "u16") + (("hdr",) if what == "grade" else ()))
    plain = _rendered("tilt", "a", 0.3)
    assert (got["map"]["u8"] != plain["u8"]).any()           # the setting changed the rows


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(hip_lib):
    from bhr_amd import HipRenderer, _lib
    from bhr_amd.disk_v2 import DiskV2Params
    lib = hip_lib
    view, v = "odd", VIEWS["odd"]
    r = _mk(view, scene="a")
    cam = r.camera_uniforms(list(v["cam"]), v["fov"])
    buf = np.zeros((v["H"], v["W"]), dtype=np.int32)

    def refused(rc, code):
        assert rc == code, (rc, lib.bhr_last_error())
        assert len(lib.bhr_last_error()) > 0 and b"raymap" in lib.bhr_last_error()

    # before a build
    refused(lib.bhr_raymap_render(r._ctx, 0.0, 0), _lib.BHR_ERR_STATE)
    refused(lib.bhr_raymap_read(r._ctx, _lib.RAYMAP_STEPS, buf.ctypes.data, buf.nbytes), _lib.BHR_ERR_STATE)
    assert r.ray_map_info()["built"] == 0
    _build(r, view)
    want = _rendered(view, "a", 0.3)

    def still_renders():
        before = r.counters()["frames_timed"]
        r.render_from_ray_map_async(t_offset=0.3)
        _assert_equal(_read(r), want, "after a refusal")
        return before

    frames = still_renders()
    # flags, t_offset, planes, sizes, null
    for rc in (lib.bhr_raymap_build(r._ctx, C.byref(cam), _lib.SKIP_BLOOM), lib.bhr_raymap_build(r._ctx, C.byref(cam), _lib.FORCE_FAST),
               lib.bhr_raymap_build(r._ctx, None, 0), lib.bhr_raymap_build(None, C.byref(cam), 0),
               lib.bhr_raymap_render(r._ctx, 0.0, _lib.SKIP_DIFFERENTIALS), lib.bhr_raymap_render(r._ctx, 0.0, _lib.PERSISTENT),
               lib.bhr_raymap_render(r._ctx, 0.0, _lib.FORCE_FAST), lib.bhr_raymap_render(r._ctx, float("nan"), 0),
               lib.bhr_raymap_render(r._ctx, float("inf"), 0), lib.bhr_raymap_render(None, 0.0, 0),
               lib.bhr_raymap_read(r._ctx, 9, buf.ctypes.data, buf.nbytes), lib.bhr_raymap_read(r._ctx, _lib.RAYMAP_STEPS, buf.ctypes.data, buf.nbytes - 4),
               lib.bhr_raymap_read(r._ctx, _lib.RAYMAP_STEPS, None, buf.nbytes)):
        refused(rc, _lib.BHR_ERR_INVALID)
    assert r.counters()["frames_timed"] == frames + 1          # nothing but still_renders' frame was launched
    still_renders()
    # the slot count
    for bad in (0, 9, -1, 8.5):
        rc = lib.bhr_set_option(r._ctx, b"raymap_slots", float(bad))
        assert rc == _lib.BHR_ERR_INVALID and b"raymap_slots" in lib.bhr_last_error()
    assert r.ray_map_info()["slots"] == 4
    still_renders()
    # ... and from the environment of bhr_create: the build refuses
    saved = os.environ.get("BHR_RAYMAP_SLOTS")
    os.environ["BHR_RAYMAP_SLOTS"] = "9"
    try:
        env = _mk(view, scene="a")
    finally:
        if saved is None:
            os.environ.pop("BHR_RAYMAP_SLOTS", None)
        else:
            os.environ["BHR_RAYMAP_SLOTS"] = saved
    refused(lib.bhr_raymap_build(env._ctx, C.byref(cam), 0), _lib.BHR_ERR_INVALID)
    assert env.ray_map_info()["built"] == 0
    env.set_option("raymap_slots", 2)
    _build(env, view)
    assert env.ray_map_info()["slots"] == 2
    env.render_from_ray_map_async(t_offset=0.3)
    _assert_equal(_read(env), want, "K = 2 after a refused build")
    env.close()
    # supersampling and adaptive supersampling: no build; the map in memory does not render until the setting is back
    for sampling in ((2, None), (2, 0.1)):
        r.set_supersample(*sampling)
        refused(lib.bhr_raymap_build(r._ctx, C.byref(cam), 0), _lib.BHR_ERR_INVALID)
        refused(lib.bhr_raymap_render(r._ctx, 0.0, 0), _lib.BHR_ERR_STATE)
        r.set_supersample(1)
        still_renders()
    # Disk V2 sources, surface and volume
    for volume in (False, True):
        r.use_disk_v2(DiskV2Params(r_in=r.r_disk_inner, r_out=r.r_disk_outer), seed=42, volume=volume)
        refused(lib.bhr_raymap_build(r._ctx, C.byref(cam), 0), _lib.BHR_ERR_INVALID)
        refused(lib.bhr_raymap_render(r._ctx, 0.0, 0), _lib.BHR_ERR_STATE)
        r.use_disk_v2(None)
        still_renders()
    # a row-block context
    sky, tex = _scene("a")
    block = HipRenderer(v["W"], v["H"], sky, tex, rows=(8, 13))
    refused(lib.bhr_raymap_build(block._ctx, C.byref(cam), 0), _lib.BHR_ERR_INVALID)
    assert b"whole-frame" in lib.bhr_last_error()
    refused(lib.bhr_raymap_render(block._ctx, 0.0, 0), _lib.BHR_ERR_INVALID)
    block.close()
    # the Python surface maps the codes as everywhere else
    with pytest.raises(ValueError):
        r.render_from_ray_map_async(t_offset=float("nan"))
    # free, render, rebuild
    r.free_ray_map()
    assert r.ray_map_info()["built"] == 0 and r.ray_map_info()["device_bytes"] == 0
    refused(lib.bhr_raymap_render(r._ctx, 0.3, 0), _lib.BHR_ERR_STATE)
    with pytest.raises(AssertionError):
        r.ray_map_passes()
    r.free_ray_map()                                     # twice: nothing to do
    np.testing.assert_array_equal(r.render(list(v["cam"]), v["fov"]), _rendered(view, "a", 0.0)["final"])
    _build(r, view)
    still_renders()
    r.close()


# ---- 8. video -------------------------------------------------------------------------------------------------------------
def test_static_camera_video_from_a_ray_map(tmp_path, hip_lib):
    from bhr_amd import drivers
    W, H, N = 48, 27, 6
    cam0, fov, speed = [6, 0, 0.5], 90, 0.1

    def video(out, **kw):
        r, _, _, _ = drivers.make_renderer(W, H, cam0, fov, n_stars=50, tex_w=256, tex_h=128, math="strict")
        try:
            drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=fov, static_cam_pos=cam0,
                                 disk_rotation_speed=speed, video_stream="off", assemble=False, **kw)
        finally:
            r.close()
        return drivers._frames_dir(out)

    d0 = video(str(tmp_path / "march" / "v.mp4"))
    d1 = video(str(tmp_path / "map" / "v.mp4"), ray_map=True)
    names = [f"frame_{f:04d}.png" for f in range(N)]
    assert sorted(os.listdir(d0)) == sorted(os.listdir(d1)) == names + ["progress.json"]
    for name in names:
        assert open(os.path.join(d0, name), "rb").read() == open(os.path.join(d1, name), "rb").read(), name
    assert open(os.path.join(d0, names[0]), "rb").read() != open(os.path.join(d0, names[-1]), "rb").read()     # the disk evolves
    p0, p1 = (json.load(open(os.path.join(d, "progress.json")))["params"] for d in (d0, d1))
    assert "ray_map" not in p0 and p1 == dict(p0, ray_map=True)
    with pytest.raises(ValueError, match="orbit"):
        video(str(tmp_path / "orbit" / "v.mp4"), ray_map=True, orbit=True)
    assert not os.path.exists(drivers._frames_dir(str(tmp_path / "orbit" / "v.mp4")))
